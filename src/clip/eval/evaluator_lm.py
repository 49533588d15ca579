"""`python -m src.clip.eval.evaluator_lm ...`: text-to-text retrieval of a sentence encoder (E5, GTE); `--model_name` is a local directory."""
from knowledge_enhanced_multimodal_retrieval_amd.evaluators import (  # noqa: F401
    evaluate_text_model, evaluate_text_model_for_training, seed_worker)
from knowledge_enhanced_multimodal_retrieval_amd.evaluators import main_text_lm as main  # noqa: F401
from knowledge_enhanced_multimodal_retrieval_amd.sentence_model import SentenceEncoder as SentenceTransformer  # noqa: F401

if __name__ == "__main__":
    main()
