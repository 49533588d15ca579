"""Reference module path `src.clip.train.trainer` -> the head trainer on frozen towers (HIP-backed loss and encoders).

    python -m src.clip.train.trainer --freeze_encoders --output_dir runs --experiment_name heads [the reference's arguments]
    python -m src.clip.train.trainer --lock_image_tower --output_dir runs --experiment_name lit [the reference's arguments]

--lock_image_tower trains the whole text tower as well, on a locked image tower (tower_train.py: attention backward in the HIP
library).  With neither flag the command exits with a message: end-to-end fine-tuning is not served."""
import sys

from knowledge_enhanced_multimodal_retrieval_amd.finetune import (  # noqa: F401
    HeadTrainer, ProjectionHeads, build_optimizer, build_parser, cache_image_pooled, cache_pooled, main)
from knowledge_enhanced_multimodal_retrieval_amd.tower_train import LockedImageTuning, TextTower, TextTowerTrainer  # noqa: F401

if __name__ == "__main__":
    sys.exit(main())
