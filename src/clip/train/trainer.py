"""Reference module path `src.clip.train.trainer` -> the head trainer on frozen towers (HIP-backed loss and encoders).

    python -m src.clip.train.trainer --freeze_encoders --output_dir runs --experiment_name heads [the reference's arguments]

Without --freeze_encoders the command exits with a message: end-to-end fine-tuning is not served."""
import sys

from knowledge_enhanced_multimodal_retrieval_amd.finetune import (  # noqa: F401
    HeadTrainer, ProjectionHeads, build_optimizer, build_parser, cache_pooled, main)

if __name__ == "__main__":
    sys.exit(main())
