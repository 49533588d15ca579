"""Reference module path `src.clip.train.losses` -> HIP-backed implementation."""
from knowledge_enhanced_multimodal_retrieval_amd.losses import InfoNCELoss, JointContrastiveLoss  # noqa: F401
