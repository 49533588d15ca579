"""Reference module path `src.clip.train.trainer` -> the head trainer on frozen towers (HIP-backed loss and encoders).

    python -m src.clip.train.trainer --freeze_encoders --output_dir runs --experiment_name heads [the reference's arguments]
    python -m src.clip.train.trainer --lock_image_tower --output_dir runs --experiment_name lit [the reference's arguments]
    python -m src.clip.train.trainer --end_to_end --output_dir runs --experiment_name e2e [the reference's arguments]

--lock_image_tower trains the whole text tower as well, on a locked image tower (tower_train.py: attention backward in the HIP
library).  --end_to_end trains both towers, the reference's recipe (attention, LayerNorm and activation backward in the HIP library).
--packed_texts (with either of these two) runs the text tower on packed texts, every text up to its own end-of-text token, instead
of the batch's longest text; it is refused with --freeze_encoders.  With none of the three flags the command exits with the message it always had."""
import sys

from knowledge_enhanced_multimodal_retrieval_amd.finetune import (  # noqa: F401
    HeadTrainer, ProjectionHeads, build_optimizer, build_parser, cache_image_pooled, cache_pixels, cache_pooled, main)
from knowledge_enhanced_multimodal_retrieval_amd.tower_train import (  # noqa: F401
    EndToEndTrainer, EndToEndTuning, LockedImageTuning, TextTower, TextTowerTrainer, VisionTower)

if __name__ == "__main__":
    sys.exit(main())
