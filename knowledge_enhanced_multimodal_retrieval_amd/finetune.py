"""Fine-tune the projection heads on frozen towers (reference ``src/clip/train/trainer.py`` with ``freeze_clip_encoders``' intent).

With the towers frozen, the pooled tower rows are constants of the dataset: ``cache_pooled`` computes them once with the engine's
encoders (``CLIP.encode_image_pooled`` / ``encode_text_pooled``), and what is left to train is, per tower, a LayerNorm, a projection and
the L2 normalisation -- ``ProjectionHeads``, plain fp32 torch autograd on ``[n, width]`` tensors -- under the joint contrastive loss, which
runs in the fused InfoNCE kernels (``losses.py``).  A batch can therefore be the whole split (``batch_size=0``).

``ProjectionHeads`` holds the MODEL'S OWN parameters (``visual.ln_post.*``, ``visual.proj``, ``ln_final.*``, ``text_projection``): an optimizer
step changes the model, ``CLIP._fingerprint`` sees the version counters move and the engine re-packs at the next ``encode_*`` call, which
is what the per-epoch validation (``evaluate_clip_model_for_training``, engine path) exercises.  Unlike ``clip_model.freeze_clip_encoders``
-- which, like the reference, leaves every visual parameter whose name contains ``proj`` trainable, the blocks' ``in_proj`` / ``out_proj`` /
``c_proj`` included -- exactly those six tensors are trainable here; ``ProjectionHeads`` sets ``requires_grad`` itself.

``HeadTrainer`` follows the reference ``CLIPTrainer`` (trainer.py:144-356): shuffled batches with the incomplete last one dropped, gradient
accumulation, ``grad_clip``, AdamW + cosine schedule as ``main_worker`` builds them (``build_optimizer``), per-epoch validation with
``val_mrr_avg``, early stopping, ``metrics_epoch.jsonl``, ``checkpoint_latest.pt`` / ``checkpoint_best.pt`` through
``clip_model.save_checkpoint`` (the full state dict: ``load_clip_model(name, checkpoint)`` and every evaluator take the result).  One
difference in the bookkeeping: ``train_loss`` is the mean of the batches' losses; the reference multiplies each by
``gradient_accumulation_steps`` on the way (trainer.py:208).  Single process, fp32; ``--mixed_precision`` is accepted and ignored.

``--lock_image_tower`` (an alternative to ``--freeze_encoders``; ``tower_train.py``) trains the whole TEXT tower as well: the image tower
stays locked -- its pooled rows are cached once (``cache_image_pooled``) -- and queries and targets of every batch run through a
differentiable restatement of the text tower whose attention is ``kemr_op_attention`` forward and ``kemr_op_attention_backward``
backward.  The loop, the loss, the validation through the served engine and the checkpoints are this module's.

``--end_to_end`` (the third mode; ``tower_train.py``) trains both towers, the reference's own recipe: the preprocessed pixels of the
training split are collected once in pinned host memory (``cache_pixels``), every batch runs through differentiable restatements of
both towers (attention, LayerNorm and the MLP activation in the HIP library in both directions, vendor GEMMs under bf16 autocast over
fp32 master weights), and ``logit_scale`` stays out of the graph.  ``--packed_texts`` (with either of these two modes) runs the text
tower on packed texts, every text up to its own end-of-text token (``TextTower(packed=True)``); it is refused with
``--freeze_encoders``, where no text tower trains.  With none of the three flags the command still exits with
``NOT_SERVED``, word for word as before.
"""
from __future__ import annotations

import argparse
import logging
import random
import sys
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .clip_model import _unwrap, load_clip_model, save_checkpoint
from .logging_utils import log_metrics_to_jsonl

logger = logging.getLogger(__name__)

HEAD_PARAMETERS = ("visual.ln_post.weight", "visual.ln_post.bias", "visual.proj", "ln_final.weight", "ln_final.bias", "text_projection")
NOT_SERVED = ("end-to-end fine-tuning is not served: there is no backward pass through the towers. Pass --freeze_encoders to train "
              "the projection heads (visual.ln_post, visual.proj, ln_final, text_projection) on frozen towers.")


def project(rows: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor, proj: torch.Tensor, eps: float) -> torch.Tensor:
    """LayerNorm -> projection -> x / ||x|| in the dtype of the arguments: one head's arithmetic."""
    x = F.layer_norm(rows, (rows.shape[-1],), ln_weight, ln_bias, eps) @ proj
    return x / x.norm(dim=-1, keepdim=True)


class ProjectionHeads(nn.Module):
    """The trainable part of a CLIP model whose towers are frozen; see the module docstring."""

    def __init__(self, model: nn.Module):
        super().__init__()
        m = _unwrap(model)
        family = getattr(getattr(m, "arch", None), "family", "clip")
        if family != "clip" or not hasattr(m.visual, "proj"):
            raise ValueError(f"ProjectionHeads: only the CLIP family has LayerNorm + projection heads (this model's family: {family!r}; "
                             "SigLIP's head is the attention pool, BERT has none)")
        for p in m.parameters():
            p.requires_grad = False
        self.ln_post, self.ln_final = m.visual.ln_post, m.ln_final                     # the model's own modules and parameters
        self.visual_proj, self.text_projection = m.visual.proj, m.text_projection
        for p in self.parameters():
            p.requires_grad = True

    def named_head_parameters(self) -> Dict[str, nn.Parameter]:
        """The six tensors under their names in the model's state dict."""
        return dict(zip(HEAD_PARAMETERS, (self.ln_post.weight, self.ln_post.bias, self.visual_proj, self.ln_final.weight,
                                          self.ln_final.bias, self.text_projection)))

    def image(self, pooled: torch.Tensor) -> torch.Tensor:
        return project(pooled.float(), self.ln_post.weight, self.ln_post.bias, self.visual_proj, self.ln_post.eps)

    def text(self, pooled: torch.Tensor) -> torch.Tensor:
        return project(pooled.float(), self.ln_final.weight, self.ln_final.bias, self.text_projection, self.ln_final.eps)

    def forward(self, pooled_image: torch.Tensor, pooled_query: torch.Tensor, pooled_target: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.image(pooled_image), self.text(pooled_query), self.text(pooled_target)


@torch.no_grad()
def cache_pooled(model: nn.Module, dataset, batch_size: int = 64, seed: int = 42, num_workers: int = 0,
                 tokenize_fn: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One pass over `dataset` (items image / query / target / uuid, the evaluators' loader): the pooled rows of the frozen towers as
    three fp32 device tensors [N, v_width], [N, t_width], [N, t_width]."""
    return _cache(model, dataset, batch_size, seed, num_workers, tokenize_fn, text_pooled=True)


@torch.no_grad()
def cache_image_pooled(model: nn.Module, dataset, batch_size: int = 64, seed: int = 42, num_workers: int = 0,
                       tokenize_fn: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``cache_pooled``'s image half for a locked image tower (``tower_train.py``): the pooled image rows fp32 [N, v_width] and, in place
    of the text rows, the token ids of queries and targets, int32 [N, ctx] each, all on the model's device."""
    return _cache(model, dataset, batch_size, seed, num_workers, tokenize_fn, text_pooled=False)


@torch.no_grad()
def cache_pixels(model: nn.Module, dataset, batch_size: int = 64, seed: int = 42, num_workers: int = 0,
                 tokenize_fn: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One pass of the evaluators' loader for ``--end_to_end`` (``tower_train.EndToEndTrainer``): the preprocessed pixels fp32
    [N, 3, S, S] and the token ids of queries and targets, int32 [N, ctx] each, all on the HOST -- the pixels in pinned memory where the
    model sits on a GPU (602 KB per 224 px image).  Where the loader yields ``PackedRaw`` the transform runs on the GPU, like ``_cache``."""
    from .evaluators import eval_loader, model_tokenize
    from .preprocess import PackedRaw, gpu_preprocess_for
    m = _unwrap(model)
    device = next(m.parameters()).device
    loader = eval_loader(dataset, batch_size, seed, num_workers, tokenize_fn or model_tokenize(m), pin=device.type == "cuda")
    img, qry, tgt = [], [], []
    gpu_pre = None
    for images, q_ids, t_ids, _ in loader:
        if isinstance(images, PackedRaw):
            gpu_pre = gpu_pre or gpu_preprocess_for(m, device)
            images = gpu_pre.batch(images)
        img.append(images.float().cpu())
        qry.append(q_ids.to(device="cpu", dtype=torch.int32))
        tgt.append(t_ids.to(device="cpu", dtype=torch.int32))
    pixels = torch.cat(img)
    return (pixels.pin_memory() if device.type == "cuda" else pixels), torch.cat(qry), torch.cat(tgt)


def _cache(model, dataset, batch_size, seed, num_workers, tokenize_fn, text_pooled: bool):
    from . import engine
    from .evaluators import eval_loader, model_tokenize
    from .preprocess import PackedRaw, gpu_preprocess_for
    m = _unwrap(model)
    m.eval()
    device = next(m.parameters()).device
    loader = eval_loader(dataset, batch_size, seed, num_workers, tokenize_fn or model_tokenize(m), pin=device.type == "cuda")
    img, qry, tgt = [], [], []
    gpu_pre = None
    for images, q_ids, t_ids, _ in loader:
        if isinstance(images, PackedRaw):
            gpu_pre = gpu_pre or gpu_preprocess_for(m, device)
            images = gpu_pre.batch(images)
        img.append(m.encode_image_pooled(images.to(device, non_blocking=True)))
        if not text_pooled:
            qry.append(q_ids.to(device=device, dtype=torch.int32, non_blocking=True))
            tgt.append(t_ids.to(device=device, dtype=torch.int32, non_blocking=True))
            continue
        n = q_ids.shape[0]
        lens = torch.cat([engine.text_lengths(q_ids.cpu()), engine.text_lengths(t_ids.cpu())])       # host lengths: no device sync
        both = m.encode_text_pooled(torch.cat([q_ids, t_ids]).to(device, non_blocking=True), lens=lens)
        qry.append(both[:n])
        tgt.append(both[n:])
    return torch.cat(img), torch.cat(qry), torch.cat(tgt)


def build_optimizer(heads: nn.Module, lr: float, weight_decay: float, num_epochs: int):
    """AdamW and the cosine schedule as the reference's main_worker builds them (trainer.py:478-492), over the trainable tensors."""
    params = [p for p in heads.parameters() if p.requires_grad]
    optimizer = torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, betas=(0.9, 0.98), eps=1e-6)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=num_epochs, eta_min=lr * 0.1)
    return optimizer, scheduler


def batch_schedule(n: int, batch_size: int, generator: torch.Generator) -> List[torch.Tensor]:
    """One epoch's batches: a seeded permutation cut into `batch_size` items, the incomplete last batch dropped (the reference's
    DataLoader(shuffle=True, drop_last=True)).  batch_size 0, or one that the split does not fill once: the whole split as one batch."""
    perm = torch.randperm(n, generator=generator)
    if batch_size <= 0 or batch_size >= n:
        return [perm]
    return [perm[s:s + batch_size] for s in range(0, n - batch_size + 1, batch_size)]


class HeadTrainer:
    """The reference CLIPTrainer's loop on cached pooled rows.  `loss_fn(image, query, target) -> (loss, metrics)` with the keys of
    JointContrastiveLoss; `validate_fn(model) -> metrics` defaults to evaluate_clip_model_for_training on `val_eval_dataset`."""

    def __init__(self, model: nn.Module, heads: ProjectionHeads, pooled: Sequence[torch.Tensor], loss_fn, optimizer, scheduler=None,
                 val_eval_dataset=None, output_dir: str = ".", total_epochs: int = 20, batch_size: int = 64,
                 early_stopping_patience: int = 5, early_stopping_metric: str = "avg", grad_clip: float = 1.0,
                 gradient_accumulation_steps: int = 1, seed: int = 42, validate_fn: Optional[Callable] = None,
                 tokenize_fn: Optional[Callable] = None):
        if early_stopping_metric not in ("avg", "t2i", "t2t"):
            raise ValueError(f"early_stopping_metric must be avg, t2i or t2t, got {early_stopping_metric!r}")
        if gradient_accumulation_steps < 1:
            raise ValueError("gradient_accumulation_steps must be >= 1")
        self.model, self.heads, self.loss_fn, self.optimizer, self.scheduler = model, heads, loss_fn, optimizer, scheduler
        self.pooled_image, self.pooled_query, self.pooled_target = pooled
        self.val_eval_dataset, self.validate_fn, self.tokenize_fn = val_eval_dataset, validate_fn, tokenize_fn
        self.output_dir = Path(output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.metrics_file = self.output_dir / "metrics_epoch.jsonl"
        self.total_epochs, self.batch_size = total_epochs, batch_size
        self.early_stopping_patience, self.early_stopping_metric = early_stopping_patience, early_stopping_metric
        self.grad_clip, self.gradient_accumulation_steps = grad_clip, gradient_accumulation_steps
        self.generator = torch.Generator().manual_seed(seed)
        self.best_metric, self.best_epoch, self.patience_counter = float("-inf"), 0, 0
        self.optimizer_steps = 0
        self.step_losses: List[float] = []

    def train_epoch(self, epoch: int) -> Dict[str, float]:
        self.heads.train()
        total = {"loss": 0.0, "loss_t2i": 0.0, "loss_t2t": 0.0}
        batches = batch_schedule(self.pooled_image.shape[0], self.batch_size, self.generator)
        accum = self.gradient_accumulation_steps
        self.optimizer.zero_grad()
        for batch_idx, idx in enumerate(batches):
            idx = idx.to(self.pooled_image.device)
            feats = self.heads(self.pooled_image[idx], self.pooled_query[idx], self.pooled_target[idx])
            loss, metrics = self.loss_fn(*feats)
            (loss / accum).backward()
            if (batch_idx + 1) % accum == 0:
                if self.grad_clip > 0:
                    torch.nn.utils.clip_grad_norm_([p for p in self.heads.parameters() if p.requires_grad], self.grad_clip)
                self.optimizer.step()
                self.optimizer.zero_grad()
                self.optimizer_steps += 1
            for k in total:
                total[k] += metrics[k]
            self.step_losses.append(metrics["loss"])
            if batch_idx % 100 == 0:
                logger.info(f"Epoch {epoch + 1} [{batch_idx}/{len(batches)}] Loss: {metrics['loss']:.4f} "
                            f"(T2I: {metrics['loss_t2i']:.4f}, T2T: {metrics['loss_t2t']:.4f})")
        n = max(len(batches), 1)
        return {"train_loss": total["loss"] / n, "train_loss_t2i": total["loss_t2i"] / n, "train_loss_t2t": total["loss_t2t"] / n}

    @torch.no_grad()
    def validate(self, epoch: int) -> Dict[str, float]:
        if self.validate_fn is not None:
            metrics = dict(self.validate_fn(self.model))
        elif self.val_eval_dataset is None:
            return {}
        else:
            from .evaluators import evaluate_clip_model_for_training
            device = next(_unwrap(self.model).parameters()).device
            metrics = evaluate_clip_model_for_training(model=_unwrap(self.model), dataset=self.val_eval_dataset, batch_size=64,
                                                       device=device, seed=42, tasks=["T2I", "T2T"], tokenize_fn=self.tokenize_fn)
        if self.early_stopping_metric == "avg":
            metrics["val_mrr_avg"] = (metrics["T2I_MRR"] + metrics["T2T_MRR"]) / 2.0
        else:
            metrics["val_mrr_avg"] = metrics["T2I_MRR" if self.early_stopping_metric == "t2i" else "T2T_MRR"]
        return metrics

    def note_epoch(self, epoch: int, current_metric: float) -> Tuple[bool, bool]:
        """Early-stopping bookkeeping of one epoch: (is this the best epoch so far, stop now)."""
        is_best = current_metric > self.best_metric
        if is_best:
            self.best_metric, self.best_epoch, self.patience_counter = current_metric, epoch, 0
        else:
            self.patience_counter += 1
        return is_best, self.patience_counter >= self.early_stopping_patience

    def save(self, epoch: int, is_best: bool) -> None:
        latest = self.output_dir / "checkpoint_latest.pt"
        save_checkpoint(self.model, self.optimizer, epoch, self.best_metric, self.best_epoch, str(latest), self.scheduler)
        if is_best:
            save_checkpoint(self.model, self.optimizer, epoch, self.best_metric, self.best_epoch,
                            str(self.output_dir / "checkpoint_best.pt"), self.scheduler)

    def train(self) -> Dict[str, float]:
        epoch_metrics: Dict[str, float] = {}
        for epoch in range(self.total_epochs):
            train_metrics = self.train_epoch(epoch)
            if self.scheduler:
                self.scheduler.step()
            val_metrics = self.validate(epoch)
            epoch_metrics = {**train_metrics, **val_metrics, "epoch": epoch, "lr": self.optimizer.param_groups[0]["lr"]}
            log_metrics_to_jsonl(epoch_metrics, str(self.metrics_file))
            logger.info(f"Epoch {epoch + 1} Summary: Train Loss: {train_metrics['train_loss']:.4f}"
                        + (f", Val Avg MRR: {val_metrics['val_mrr_avg']:.2f}%" if val_metrics else ""))
            is_best, stop = self.note_epoch(epoch, val_metrics.get("val_mrr_avg", float("-inf")))
            self.save(epoch, is_best)
            if stop:
                logger.info(f"Early stopping triggered! Best epoch: {self.best_epoch}")
                break
        logger.info(f"Training complete! Best MRR: {self.best_metric:.2f}% (Epoch {self.best_epoch})")
        return epoch_metrics


# ------------------------------------------------------------------------------------------------ CLI (src/clip/train/trainer.py)
def build_parser() -> argparse.ArgumentParser:
    """The reference's arguments (trainer.py:532-580) plus the three modes, --synthetic and --dataset."""
    parser = argparse.ArgumentParser(description="Fine-tune CLIP with the joint T2I + T2T loss: the projection heads on frozen towers, the "
                                                 "text tower on a locked image tower, or both towers end to end")
    parser.add_argument("--model_name", type=str, default="ViT-L/14")
    parser.add_argument("--checkpoint", type=str, default=None, help="Path to checkpoint to start from")
    parser.add_argument("--images_dir", type=str, default=None, help="accepted for the shipped scripts; the data come from --dataset")
    parser.add_argument("--texts_dir", type=str, default=None, help="accepted for the shipped scripts; the data come from --dataset")
    parser.add_argument("--max_text_length", type=int, default=150, help="Maximum text length in words")
    parser.add_argument("--temperature", type=float, default=0.07)
    parser.add_argument("--t2i_weight", type=float, default=0.5, help="Weight for T2I loss")
    parser.add_argument("--t2t_weight", type=float, default=0.5, help="Weight for T2T loss")
    parser.add_argument("--batch_size", type=int, default=64, help="items per contrastive batch; 0 = the whole training split in one batch")
    parser.add_argument("--num_epochs", type=int, default=20)
    parser.add_argument("--lr", type=float, default=1e-5)
    parser.add_argument("--weight_decay", type=float, default=0.01)
    parser.add_argument("--grad_clip", type=float, default=1.0)
    parser.add_argument("--gradient_accumulation_steps", type=int, default=1, help="Number of gradient accumulation steps")
    parser.add_argument("--early_stopping_patience", type=int, default=5)
    parser.add_argument("--early_stopping_metric", type=str, default="avg", choices=["avg", "t2i", "t2t"])
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("--mixed_precision", action="store_true", help="accepted and ignored: the heads train in fp32")
    parser.add_argument("--output_dir", type=str, required=True)
    parser.add_argument("--experiment_name", type=str, required=True)
    parser.add_argument("--use_wandb", action="store_true", help="accepted and ignored")
    parser.add_argument("--wandb_project", type=str, default="clip-art-retrieval")
    parser.add_argument("--seed", type=int, default=42)
    mode = parser.add_mutually_exclusive_group()
    mode.add_argument("--freeze_encoders", action="store_true",
                      help="train the projection heads on frozen towers (one of this, --lock_image_tower and --end_to_end is required)")
    mode.add_argument("--lock_image_tower", action="store_true",
                      help="instead of --freeze_encoders: train the projection heads AND the whole text tower on a locked image tower "
                           "(cached pooled image rows; attention backward in the HIP library); needs a batch size")
    mode.add_argument("--end_to_end", action="store_true",
                      help="instead of --freeze_encoders: train both towers and the projection heads, the reference's recipe (pixels cached "
                           "in pinned host memory; attention, LayerNorm and activation backward in the HIP library); needs a batch size")
    parser.add_argument("--packed_texts", action="store_true",
                        help="with --lock_image_tower or --end_to_end: run the text tower on packed texts, every text up to its own "
                             "end-of-text token instead of the batch's longest text (packed attention forward and backward in the HIP "
                             "library); the default is off")
    parser.add_argument("--synthetic", type=int, default=0, metavar="N",
                        help="train and validate on N seeded synthetic items each instead of the HuggingFace dataset (offline)")
    parser.add_argument("--dataset", type=str, default="xuemduan/reevaluate-image-text-pairs")
    return parser


PACKED_TEXTS_REFUSED = ("--packed_texts is not served with --freeze_encoders: the frozen towers run once, through the served engine, "
                        "when the pooled rows are cached, and no text tower takes part in training; give it with --lock_image_tower or "
                        "--end_to_end")


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.freeze_encoders and not args.lock_image_tower and not args.end_to_end:
        print(f"error: {NOT_SERVED}", file=sys.stderr)
        return 2
    if args.packed_texts and args.freeze_encoders:
        parser.error(PACKED_TEXTS_REFUSED)
    if args.end_to_end and args.batch_size <= 0:
        from .tower_train import BATCH_0_REFUSED_END_TO_END
        parser.error(BATCH_0_REFUSED_END_TO_END)
    if args.lock_image_tower and args.batch_size <= 0:
        from .tower_train import BATCH_0_REFUSED
        parser.error(BATCH_0_REFUSED)
    from . import clip_api, tokenizer
    from .datasets import CLIPEvalDatasetHF, SyntheticRetrievalDataset
    from .logging_utils import setup_logger
    from .losses import JointContrastiveLoss
    out = Path(args.output_dir) / args.experiment_name
    out.mkdir(parents=True, exist_ok=True)
    setup_logger(__name__, str(out / "train.log"))
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    if args.synthetic > 0:           # synthetic data: seeded random weights / hash token ids are acceptable
        clip_api.allow_random_weights(True)
        tokenizer.allow_hash_tokenizer(True)
    device = "cuda:0"
    model, preprocess = load_clip_model(model_name=args.model_name, checkpoint_path=args.checkpoint, device=device)
    model = model.float()
    if args.synthetic > 0:
        train_set = SyntheticRetrievalDataset(args.synthetic, model.arch.image_size, args.seed)
        val_set = SyntheticRetrievalDataset(args.synthetic, model.arch.image_size, args.seed + 1)
    else:
        from datasets import load_dataset
        ds = load_dataset(args.dataset)
        train_set = CLIPEvalDatasetHF(ds["train"], preprocess, args.max_text_length)
        val_set = CLIPEvalDatasetHF(ds["validation"], preprocess, args.max_text_length)
    workers = 0 if args.synthetic > 0 else args.num_workers
    if args.end_to_end:
        from .tower_train import EndToEndTrainer, EndToEndTuning
        logger.info(f"Collecting the preprocessed pixels of {len(train_set)} training items (end to end)...")
        pooled = cache_pixels(model, train_set, batch_size=64, seed=args.seed, num_workers=workers)
        heads, trainer_cls = EndToEndTuning(model, packed=args.packed_texts), EndToEndTrainer
    elif args.lock_image_tower:
        from .tower_train import LockedImageTuning, TextTowerTrainer
        logger.info(f"Caching the pooled image rows of {len(train_set)} training items (locked image tower)...")
        pooled = cache_image_pooled(model, train_set, batch_size=64, seed=args.seed, num_workers=workers)
        heads, trainer_cls = LockedImageTuning(model, packed=args.packed_texts), TextTowerTrainer
    else:
        logger.info(f"Caching the pooled rows of {len(train_set)} training items (frozen towers)...")
        pooled = cache_pooled(model, train_set, batch_size=64, seed=args.seed, num_workers=workers)
        heads, trainer_cls = ProjectionHeads(model), HeadTrainer
    loss_fn = JointContrastiveLoss(temperature=args.temperature, t2i_weight=args.t2i_weight, t2t_weight=args.t2t_weight)
    optimizer, scheduler = build_optimizer(heads, args.lr, args.weight_decay, args.num_epochs)
    trainer = trainer_cls(model, heads, pooled, loss_fn, optimizer, scheduler, val_eval_dataset=val_set, output_dir=str(out),
                          total_epochs=args.num_epochs, batch_size=args.batch_size, early_stopping_patience=args.early_stopping_patience,
                          early_stopping_metric=args.early_stopping_metric, grad_clip=args.grad_clip,
                          gradient_accumulation_steps=args.gradient_accumulation_steps, seed=args.seed)
    trainer.train()
    return 0


if __name__ == "__main__":
    sys.exit(main())
