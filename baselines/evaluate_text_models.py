"""Legacy five-variant text-to-text evaluation of a sentence encoder (the reference's baselines/evaluate_text_models.py): single and
multi mode; `--model_name` is a local directory."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from knowledge_enhanced_multimodal_retrieval_amd.evaluators import TextVariantsDataset as TextOnlyDataset  # noqa: E402,F401
from knowledge_enhanced_multimodal_retrieval_amd.evaluators import evaluate_text_model_variants as evaluate_text_model  # noqa: E402,F401
from knowledge_enhanced_multimodal_retrieval_amd.evaluators import main_text_variants as main  # noqa: E402,F401
from knowledge_enhanced_multimodal_retrieval_amd.evaluators import seed_worker  # noqa: E402,F401

if __name__ == "__main__":
    main()
