"""Reference module path `src.clip.train.train_fusion` -> the fusion-head trainer over a frozen CLIP (HIP-backed loss and ranking).

    python -m src.clip.train.train_fusion --model_name ViT-L/14 --clip_checkpoint C --fusion_type gated --output_dir runs/gated

The reference's file of this name is a copy of its evaluator; this one trains: it writes the fusion_best.pt that
`python -m src.clip.eval.evaluator_fusion --fusion_checkpoint` loads."""
import sys

from knowledge_enhanced_multimodal_retrieval_amd.fusion_train import (  # noqa: F401
    FusionHeadTrainer, build_parser, checkpoint_dict, main)

if __name__ == "__main__":
    sys.exit(main())
