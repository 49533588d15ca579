"""Train the learned fusion heads over a frozen CLIP (``python -m src.clip.train.train_fusion``).

The reference's ``src/clip/train/train_fusion.py`` is a copy of its evaluator and has no training loop; ``evaluator_fusion
--fusion_checkpoint F`` nevertheless loads ``F["fusion_head_state_dict"]``.  This module writes that file.  The objective is the
project's own: symmetric InfoNCE over the head's fused scores (``losses.FusionContrastiveLoss``, csrc/pairhead.hip), temperature fixed.

With the encoders frozen the three embeddings of every item are constants: both splits are encoded once through the evaluators' loader
into normalised ``[N, D]`` device tensors, and a step is one fused forward + backward over a batch of them -- the whole split when
``batch_size`` is 0, since the n x n scores are never stored.  ``FusionHeadTrainer`` has ``finetune.HeadTrainer``'s semantics: seeded
shuffled batches with the incomplete last one dropped, ``grad_clip``, AdamW + cosine schedule (``finetune.build_optimizer``), validation
after every epoch -- the SERVED ranking, ``FusionModel.rank``, MRR from ``ranking.metrics_from_ranks`` -- early stopping,
``metrics_epoch.jsonl``, ``fusion_latest.pt`` / ``fusion_best.pt``.  The head stays in eval mode: its Dropout(0.1) is not applied.
Trained: linear, gated, simple_gated, simple_gated_with_bias; bilinear and cross_attention are refused with the reason.
"""
from __future__ import annotations

import argparse
import logging
import random
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .finetune import batch_schedule, build_optimizer
from .logging_utils import log_metrics_to_jsonl
from .losses import FusionContrastiveLoss, fusion_train_mode

logger = logging.getLogger(__name__)
CHECKPOINT_KEYS = ("fusion_head_state_dict", "fusion_type", "embed_dim", "epoch", "best_metric", "optimizer_state_dict")


def checkpoint_dict(fusion_model, embed_dim: int, epoch: int, best_metric: float, optimizer) -> Dict:
    """What fusion_latest.pt / fusion_best.pt hold: the head under the reference's key, tensors on the CPU."""
    head = {k: v.detach().cpu().clone() for k, v in fusion_model.fusion_head.state_dict().items()}
    return {"fusion_head_state_dict": head, "fusion_type": fusion_model.fusion_type, "embed_dim": int(embed_dim), "epoch": int(epoch),
            "best_metric": float(best_metric), "optimizer_state_dict": optimizer.state_dict()}


class FusionHeadTrainer:
    """`train` / `val`: (query, image, target) normalised [N, D] device tensors of the frozen encoders."""

    def __init__(self, fusion_model, train: Sequence[torch.Tensor], val: Optional[Sequence[torch.Tensor]], loss_fn: FusionContrastiveLoss,
                 optimizer, scheduler=None, output_dir: str = ".", total_epochs: int = 20, batch_size: int = 0,
                 early_stopping_patience: int = 5, grad_clip: float = 1.0, seed: int = 42):
        fusion_train_mode(fusion_model.fusion_type)
        self.model, self.loss_fn, self.optimizer, self.scheduler = fusion_model, loss_fn, optimizer, scheduler
        self.train_q, self.train_img, self.train_tgt = train
        self.val = val
        self.output_dir = Path(output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.metrics_file = self.output_dir / "metrics_epoch.jsonl"
        self.total_epochs, self.batch_size = total_epochs, batch_size
        self.early_stopping_patience, self.grad_clip = early_stopping_patience, grad_clip
        self.generator = torch.Generator().manual_seed(seed)
        self.best_metric, self.best_epoch, self.patience_counter = float("-inf"), 0, 0
        self.step_losses: List[float] = []

    def train_epoch(self, epoch: int) -> Dict[str, float]:
        self.model.fusion_head.eval()                  # no dropout: the function trained is the function served
        total = {"loss": 0.0, "loss_q2g": 0.0, "loss_g2q": 0.0}
        batches = batch_schedule(self.train_q.shape[0], self.batch_size, self.generator)
        params = [p for p in self.model.fusion_head.parameters() if p.requires_grad]
        for idx in batches:
            idx = idx.to(self.train_q.device)
            self.optimizer.zero_grad()
            loss, metrics = self.loss_fn(self.model, self.train_q[idx], self.train_img[idx], self.train_tgt[idx])
            loss.backward()
            if self.grad_clip > 0:
                torch.nn.utils.clip_grad_norm_(params, self.grad_clip)
            self.optimizer.step()
            for k in total:
                total[k] += metrics[k]
            self.step_losses.append(metrics["loss"])
        n = max(len(batches), 1)
        return {"train_loss": total["loss"] / n, "train_loss_q2g": total["loss_q2g"] / n, "train_loss_g2q": total["loss_g2q"] / n}

    @torch.no_grad()
    def validate(self) -> Dict[str, float]:
        if self.val is None:
            return {}
        from . import ranking
        q, img, tgt = self.val
        ranks, _, _ = self.model.rank(q, img, tgt, k=0)
        metrics = ranking.metrics_from_ranks(ranks, [1, 5, 10, 20])
        return {f"val_{k}": v for k, v in metrics.items()}

    def note_epoch(self, epoch: int, current_metric: float) -> Tuple[bool, bool]:
        is_best = current_metric > self.best_metric
        if is_best:
            self.best_metric, self.best_epoch, self.patience_counter = current_metric, epoch, 0
        else:
            self.patience_counter += 1
        return is_best, self.patience_counter >= self.early_stopping_patience

    def save(self, epoch: int, is_best: bool) -> None:
        ckpt = checkpoint_dict(self.model, self.train_q.shape[1], epoch, self.best_metric, self.optimizer)
        torch.save(ckpt, str(self.output_dir / "fusion_latest.pt"))
        if is_best:
            torch.save(ckpt, str(self.output_dir / "fusion_best.pt"))

    def train(self) -> Dict[str, float]:
        epoch_metrics: Dict[str, float] = {}
        for epoch in range(self.total_epochs):
            train_metrics = self.train_epoch(epoch)
            if self.scheduler:
                self.scheduler.step()
            val_metrics = self.validate()
            epoch_metrics = {**train_metrics, **val_metrics, "epoch": epoch, "lr": self.optimizer.param_groups[0]["lr"]}
            log_metrics_to_jsonl(epoch_metrics, str(self.metrics_file))
            logger.info(f"Epoch {epoch + 1}: train loss {train_metrics['train_loss']:.4f}"
                        + (f", val MRR {val_metrics['val_MRR']:.2f}%" if val_metrics else ""))
            # without a validation split every epoch is "the best so far": the lower training loss wins
            current = val_metrics["val_MRR"] if val_metrics else -train_metrics["train_loss"]
            is_best, stop = self.note_epoch(epoch, current)
            self.save(epoch, is_best)
            if stop:
                logger.info(f"Early stopping triggered! Best epoch: {self.best_epoch}")
                break
        return epoch_metrics


# ------------------------------------------------------------------------------------------------ CLI (src/clip/train/train_fusion.py)
def build_parser() -> argparse.ArgumentParser:
    """evaluator_fusion's model and data arguments plus HeadTrainer's training arguments."""
    parser = argparse.ArgumentParser(description="Train a learned T2I/T2T fusion head over a frozen CLIP (symmetric InfoNCE on the fused scores)")
    parser.add_argument("--model_name", type=str, default="ViT-L/14")
    parser.add_argument("--tokenizer_dir", type=str, default=None, metavar="DIR", help="SigLIP models only: directory of the tokenizer.json")
    parser.add_argument("--clip_checkpoint", type=str, default=None)
    parser.add_argument("--fusion_checkpoint", type=str, default=None, help="start from this head (fusion_head_state_dict)")
    parser.add_argument("--fusion_type", type=str, required=True,
                        choices=["linear", "cross_attention", "gated", "simple_gated", "simple_gated_with_bias", "bilinear"])
    parser.add_argument("--images_dir", type=str, default=None, help="accepted for the shipped scripts; the data come from --dataset")
    parser.add_argument("--texts_dir", type=str, default=None, help="accepted for the shipped scripts; the data come from --dataset")
    parser.add_argument("--splits_file", type=str, default=None)
    parser.add_argument("--max_text_length", type=int, default=150)
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--output_dir", type=str, required=True)
    parser.add_argument("--synthetic", type=int, default=0, metavar="N",
                        help="train and validate on N seeded synthetic items each instead of the HuggingFace dataset (offline)")
    parser.add_argument("--dataset", type=str, default="xuemduan/reevaluate-image-text-pairs")
    parser.add_argument("--batch_size", type=int, default=0, help="items per contrastive batch; 0 = the whole training split in one batch")
    parser.add_argument("--encode_batch_size", type=int, default=64, help="items per encoder call while the splits are embedded")
    parser.add_argument("--num_epochs", type=int, default=20)
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--weight_decay", type=float, default=0.01)
    parser.add_argument("--temperature", type=float, default=0.07)
    parser.add_argument("--grad_clip", type=float, default=1.0)
    parser.add_argument("--early_stopping_patience", type=int, default=5)
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("--seed", type=int, default=42)
    return parser


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        fusion_train_mode(args.fusion_type)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    from . import clip_api, tokenizer
    from .clip_model import load_clip_model
    from .datasets import CLIPEvalDatasetHF, SyntheticRetrievalDataset
    from .evaluators import _bind_tokenizer, encode_dataset
    from .fusion_model import FusionModel
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    if args.synthetic > 0:           # synthetic data: seeded random weights / hash token ids are acceptable
        clip_api.allow_random_weights(True)
        tokenizer.allow_hash_tokenizer(True)
    clip_model, preprocess = load_clip_model(model_name=args.model_name, checkpoint_path=args.clip_checkpoint, device=args.device)
    _bind_tokenizer(clip_model, args)
    embed_dim = clip_model.arch.embed_dim
    fusion_model = FusionModel(clip_model=clip_model, fusion_type=args.fusion_type, embed_dim=embed_dim).to(args.device)
    if args.fusion_checkpoint:
        ckpt = torch.load(args.fusion_checkpoint, map_location="cpu", weights_only=True)
        fusion_model.fusion_head.load_state_dict(ckpt["fusion_head_state_dict"])
    if args.synthetic > 0:
        train_set = SyntheticRetrievalDataset(args.synthetic, clip_model.arch.image_size, args.seed)
        val_set = SyntheticRetrievalDataset(args.synthetic, clip_model.arch.image_size, args.seed + 1)
    else:
        from datasets import load_dataset
        ds = load_dataset(args.dataset)
        train_set = CLIPEvalDatasetHF(ds["train"], preprocess, args.max_text_length)
        val_set = CLIPEvalDatasetHF(ds["validation"], preprocess, args.max_text_length)
    workers = 0 if args.synthetic > 0 else args.num_workers
    splits = []
    for name, split in (("training", train_set), ("validation", val_set)):
        logger.info(f"Encoding {len(split)} {name} items once (frozen encoders)...")
        image, query, target, _ = encode_dataset(clip_model, split, args.encode_batch_size, args.seed, workers, None)
        splits.append(tuple(torch.as_tensor(t).to(args.device).float().contiguous() for t in (query, image, target)))
    optimizer, scheduler = build_optimizer(fusion_model.fusion_head, args.lr, args.weight_decay, args.num_epochs)
    trainer = FusionHeadTrainer(fusion_model, splits[0], splits[1], FusionContrastiveLoss(temperature=args.temperature), optimizer, scheduler,
                                output_dir=args.output_dir, total_epochs=args.num_epochs, batch_size=args.batch_size,
                                early_stopping_patience=args.early_stopping_patience, grad_clip=args.grad_clip, seed=args.seed)
    trainer.train()
    return 0


if __name__ == "__main__":
    sys.exit(main())
