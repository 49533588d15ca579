"""Shared cases of the fusion-head training tests (tests/test_fusion_train_host.py, test_pairhead_gpu.py, test_fusion_train_gpu.py):
seeded embeddings and heads, the dense torch formulation of the objective, and the planted-data recipe."""
import torch

from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel

HEADS = ("linear", "gated", "simple_gated", "simple_gated_with_bias")


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def triplet(n, d, seed, dtype=torch.float32):
    """(q, img, tgt) unit rows [n, d]: the query resembles its image and its target, the target its image."""
    g = torch.Generator().manual_seed(seed)
    img = unit(torch.randn(n, d, generator=g, dtype=torch.float64))
    tgt = unit(img + 1.5 * unit(torch.randn(n, d, generator=g, dtype=torch.float64)))
    q = unit(img + tgt + 4.0 * unit(torch.randn(n, d, generator=g, dtype=torch.float64)))
    return q.to(dtype), img.to(dtype), tgt.to(dtype)


def linear_params(hidden, seed):
    """(w0 [hidden, 2], b0 [hidden], w1 [hidden], b1 [1]) fp32: units on both sides of their kink over the cosines' range."""
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(hidden, 2, generator=g)
    b0 = 0.3 * torch.randn(hidden, generator=g)
    w1 = 2.0 * torch.randn(hidden, generator=g) / hidden ** 0.5
    b1 = torch.randn(1, generator=g)
    return w0.float(), b0.float(), w1.float(), b1.float()


def make_model(fusion_type, embed_dim, seed):
    """A FusionModel over no encoder whose head holds seeded non-trivial parameters."""
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=embed_dim)
    g = torch.Generator().manual_seed(seed)
    h = fm.fusion_head
    with torch.no_grad():
        if fusion_type == "linear":
            for p, v in zip((h.fusion[0].weight, h.fusion[0].bias, h.fusion[3].weight, h.fusion[3].bias), linear_params(128, seed)):
                p.copy_(v.reshape(p.shape))
        elif fusion_type == "gated":
            h.gate_net[0].weight.copy_(torch.randn(128, embed_dim, generator=g))
            h.gate_net[0].bias.copy_(0.3 * torch.randn(128, generator=g))
            h.gate_net[3].weight.copy_(0.3 * torch.randn(1, 128, generator=g))
            h.gate_net[3].bias.copy_(0.3 * torch.randn(1, generator=g))
        else:
            h.query_weight.copy_(3.0 * torch.randn(embed_dim, generator=g))
            h.bias.copy_((0.5 * torch.randn(1, generator=g)).reshape(h.bias.shape))
    return fm.eval()


def dense_scores(head, fusion_type, q, img, tgt):
    """The head's [n, n] scores in plain torch, in the dtype of the arguments (differentiable): the formulation the kernels replace."""
    t2i, t2t = q @ img.T, q @ tgt.T
    if fusion_type == "linear":
        return head.fusion(torch.stack([t2i, t2t], dim=-1)).squeeze(-1)
    g = head.gate(q).reshape(-1, 1)
    return g * t2i + (1 - g) * t2t


def symmetric_cross_entropy(scores, temperature):
    """(loss, loss_q2g, loss_g2q) of the objective from dense scores."""
    z = scores / temperature
    diag = torch.diagonal(z)
    a, b = (torch.logsumexp(z, dim=1) - diag).mean(), (torch.logsumexp(z, dim=0) - diag).mean()
    return (a + b) / 2, a, b


def dense_loss(head, fusion_type, q, img, tgt, temperature):
    return symmetric_cross_entropy(dense_scores(head, fusion_type, q, img, tgt), temperature)[0]


def head_kernel_inputs(fm, q):
    """(mode, gate, linear) as the kernels take this model's head: fp32 CPU tensors, the gate by the head's own gate()."""
    if fm.fusion_type == "linear":
        f = fm.fusion_head.fusion
        lin = (f[0].weight.detach().float().reshape(-1, 2), f[0].bias.detach().float().reshape(-1), f[3].weight.detach().float().reshape(-1),
               f[3].bias.detach().float().reshape(1))
        return 1, None, tuple(t.cpu().contiguous() for t in lin)
    with torch.no_grad():
        gate = fm.fusion_head.eval().gate(q.to(next(fm.fusion_head.parameters()).device)).reshape(-1).float().cpu()
    return 0, gate, None


def planted(n, d, seed):
    """T2T carries no signal: img = unit(randn), q = unit(img + 2.5 unit(randn)), tgt = unit(randn) -> (q, img, tgt) fp32."""
    g = torch.Generator().manual_seed(seed)
    img = unit(torch.randn(n, d, generator=g, dtype=torch.float64))
    q = unit(img + 2.5 * unit(torch.randn(n, d, generator=g, dtype=torch.float64)))
    tgt = unit(torch.randn(n, d, generator=g, dtype=torch.float64))
    return q.float(), img.float(), tgt.float()


def mrr_of_scores(scores):
    """MRR (fraction) of the diagonal under dense scores, ties counted against the ground truth."""
    s = scores.detach().double()
    ranks = (s >= torch.diagonal(s)[:, None]).sum(dim=1).clamp(min=1)
    return float((1.0 / ranks.double()).mean())
