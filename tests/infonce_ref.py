"""fp64 statement of the fused InfoNCE entry points (include/kemr.h kemr_infonce_forward / kemr_infonce_backward) and their budget.

Statement (reference src/clip/train/losses.py:41-55, fp64 torch on the CPU): z = a b^T / tau,
    loss_a2b = mean_i (lse_j z_ij - z_ii),  loss_b2a = mean_j (lse_i z_ij - z_jj),  loss = (loss_a2b + loss_b2a) / 2,
    G = dL/dz = (P + Q) / (2 n) - I / n  (P = softmax over rows, Q = softmax over columns),  grad_a = G b / tau,  grad_b = G^T a / tau.
`joint` is the reference's JointContrastiveLoss on top: w_t2i InfoNCE(target, image) + w_t2t InfoNCE(query, target), weights normalised.

Budget (u = 2^-24; every bound is an fp64 tensor that `oracle.rounding.check_budget(got, ref, extra, fmt="fp32")` takes as `extra`).

1. Scores.  The kernels contract bf16 pairs, hi.hi + lo.hi + hi.lo with fp32 accumulation: the arithmetic of the terms == 3 similarity
   panels.  `oracle.rounding.panel_representation_bound` bounds what the split costs (c sum |a||b|, c = 3 2^-16 + ...), and the MFMA
   K loop's accumulation is the accumulator bar of tests/test_numerics_sim_gpu.py, KAPPA u sum |hi||hi| + |lo||hi| + |hi||lo| <=
   KAPPA u (1 + 2^-7) sum |a||b| (KAPPA = 10 there and here).  e_s = their sum, per entry.
2. Logits.  z = fl(s fl(1 / tau)): two fp32 roundings, and the score error times 1 / tau:  e_z = e_s / tau + 3 u |z|.  E = max e_z.
3. Log-sum-exp.  Moving every logit of a row by at most E moves the row's lse by at most E.  On top, in fp32: each term
   exp2((z - m) log2e) carries the subtraction's and the product's rounding, 2 u |z - m| <= 2 u R (R = max z - min z of the matrix),
   and v_exp_f32's ulp; the sum of n positive terms at most (n - 1) u relative whatever its order, the rescales of the online maximum
   and the merge of the partial sums a few u more (16 u covers 2 per tile and chunk at the sizes tested); m + log(sum) rounds once and
   logf costs 2 ulp.  e_lse = E + u (2 R + n + 20) + 3 u |lse|.
4. Loss.  Each term lse_i - z_ii moves by e_lse_i + e_z_ii + u |term|; the mean is an fp64 sum on the device, rounded once (the half
   ulp check_budget grants): e_loss = mean of those; the total is the mean of the two halves' bounds.
5. dL/dz.  P_ij = exp(z_ij - lse_i) moves by its own size times expm1(2 E') (logit and lse both move, E' = E plus the fp32 lse terms
   of 3) plus u (2 |z - lse| + 3) for the subtraction, the product with log2e and v_exp_f32, and at most 2^-126 absolute where the
   result is flushed; the same for Q.  The sum, the product with fl(0.5 / n) and the diagonal's - fl(1 / n) round once each:
   e_G = (P f_P + Q f_Q) / (2 n) + 3 u (P + Q) / (2 n) + [i = j] 2 u / n + 2^-126.
6. Gradients.  grad = (G b) / tau with G and b as bf16 pairs again: sum_j e_G |b| for what G itself carries, the split's c sum |G'||b|
   (panel_representation_bound again, |G'| <= |G| + e_G) and the accumulator bar KAPPA u (1 + 2^-7) sum |G'||b|, all times 1 / tau,
   and 3 u |grad| for the product with fl(1 / tau).

Nothing here is fitted to the device's output: the constants are the formats' (u, c), the accumulator bar the similarity tests already
hold the same MFMA loop to, and counts of roundings.  The worst measured ratios are in DESIGN.md ("Fused InfoNCE").
"""
import torch

from oracle import rounding as R

U = 2.0 ** -24
KAPPA = 10                  # tests/test_numerics_sim_gpu.py KAPPA: the accumulator bar of the 16x16x32 bf16 MFMA K loop
TINY = 2.0 ** -126


def infonce(a, b, temperature):
    """fp64 statement: dict with loss, loss_a2b, loss_b2a (0-d), lse_rows, lse_cols [n], grad_a, grad_b [n, d] (of `loss`), and z, P, Q."""
    a, b = a.double().cpu(), b.double().cpu()
    n = a.shape[0]
    z = (a @ b.T) / temperature
    lse_r, lse_c = torch.logsumexp(z, dim=1), torch.logsumexp(z, dim=0)
    diag = torch.diagonal(z)
    l_ab, l_ba = (lse_r - diag).mean(), (lse_c - diag).mean()
    P, Q = torch.exp(z - lse_r[:, None]), torch.exp(z - lse_c[None, :])
    G = (P + Q) / (2 * n) - torch.eye(n, dtype=torch.float64) / n
    return {"loss": (l_ab + l_ba) / 2, "loss_a2b": l_ab, "loss_b2a": l_ba, "lse_rows": lse_r, "lse_cols": lse_c,
            "grad_a": (G @ b) / temperature, "grad_b": (G.T @ a) / temperature, "z": z, "P": P, "Q": Q, "G": G}


def joint(image, query, target, temperature, t2i_weight, t2t_weight):
    """fp64 statement of JointContrastiveLoss and its three gradients (the target's is the sum over both pairs)."""
    s = t2i_weight + t2t_weight
    wi, wt = t2i_weight / s, t2t_weight / s
    t2i, t2t = infonce(target, image, temperature), infonce(query, target, temperature)
    return {"loss": wi * t2i["loss"] + wt * t2t["loss"], "loss_t2i": t2i["loss"], "loss_t2t": t2t["loss"],
            "t2i_weight": wi, "t2t_weight": wt, "grad_image": wi * t2i["grad_b"], "grad_query": wt * t2t["grad_a"],
            "grad_target": wi * t2i["grad_a"] + wt * t2t["grad_b"], "t2i": t2i, "t2t": t2t}


def budget(a, b, temperature, ref=None):
    """The bounds of the module docstring for one call: dict of `extra` tensors named like infonce()'s entries."""
    a, b = a.double().cpu(), b.double().cpu()
    ref = infonce(a, b, temperature) if ref is None else ref
    n = a.shape[0]
    z, P, Q, G = ref["z"], ref["P"], ref["Q"], ref["G"]
    ab = a.abs() @ b.abs().T
    _, split = R.panel_representation_bound([a], [b], 3)
    e_z = (split + KAPPA * U * (1 + 2.0 ** -7) * ab) / temperature + 3 * U * z.abs()                  # 1, 2
    E = float(e_z.max())
    lse_fp = U * (2 * float(z.max() - z.min()) + n + 20)
    e_lse_r = E + lse_fp + 3 * U * ref["lse_rows"].abs()                                                # 3
    e_lse_c = E + lse_fp + 3 * U * ref["lse_cols"].abs()
    diag, e_diag = torch.diagonal(z), torch.diagonal(e_z)
    e_ab = (e_lse_r + e_diag + U * (ref["lse_rows"] - diag).abs()).mean()                              # 4
    e_ba = (e_lse_c + e_diag + U * (ref["lse_cols"] - diag).abs()).mean()
    f_p = torch.expm1(torch.tensor(2 * E + lse_fp + 3 * U, dtype=torch.float64) + 3 * U * ref["lse_rows"].abs())[:, None] \
        + U * (2 * (z - ref["lse_rows"][:, None]).abs() + 3)                                            # 5
    f_q = torch.expm1(torch.tensor(2 * E + lse_fp + 3 * U, dtype=torch.float64) + 3 * U * ref["lse_cols"].abs())[None, :] \
        + U * (2 * (z - ref["lse_cols"][None, :]).abs() + 3)
    e_G = (P * f_p + Q * f_q) / (2 * n) + 3 * U * (P + Q) / (2 * n) + torch.eye(n, dtype=torch.float64) * (2 * U / n) + TINY
    Gp = G.abs() + e_G

    def grad_extra(Gm, eG, other, grad):                                                                # 6
        _, c_split = R.panel_representation_bound([Gm], [other.T.contiguous()], 3)
        return (eG @ other.abs() + c_split + KAPPA * U * (1 + 2.0 ** -7) * (Gm @ other.abs())) / temperature + 3 * U * grad.abs()

    return {"loss": (e_ab + e_ba) / 2, "loss_a2b": e_ab, "loss_b2a": e_ba, "lse_rows": e_lse_r, "lse_cols": e_lse_c,
            "grad_a": grad_extra(Gp, e_G, b, ref["grad_a"]), "grad_b": grad_extra(Gp.T.contiguous(), e_G.T.contiguous(), a, ref["grad_b"])}


def joint_budget(image, query, target, temperature, t2i_weight, t2t_weight, ref=None):
    """Bounds for JointContrastiveLoss through autograd: the weighted sums of the two calls' bounds, plus u per fp32 product / sum that
    torch adds (the weights' products, the sum of the two losses, the sum of the target's two gradients)."""
    ref = joint(image, query, target, temperature, t2i_weight, t2t_weight) if ref is None else ref
    wi, wt = ref["t2i_weight"], ref["t2t_weight"]
    bi = budget(target, image, temperature, ref["t2i"])
    bt = budget(query, target, temperature, ref["t2t"])
    return {"loss": wi * bi["loss"] + wt * bt["loss"] + 3 * U * (abs(ref["loss_t2i"]) + abs(ref["loss_t2t"])),
            "loss_t2i": bi["loss"], "loss_t2t": bt["loss"],
            "grad_image": wi * bi["grad_b"] + 2 * U * ref["grad_image"].abs(),
            "grad_query": wt * bt["grad_a"] + 2 * U * ref["grad_query"].abs(),
            "grad_target": wi * bi["grad_a"] + wt * bt["grad_b"]
            + 3 * U * (wi * ref["t2i"]["grad_a"].abs() + wt * ref["t2t"]["grad_b"].abs())}
