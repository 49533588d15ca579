"""fp64 statement of the fused pair-score contrastive loss (include/kemr.h kemr_pairhead_forward / kemr_pairhead_backward) and its budget.

Statement (fp64 torch on the CPU): t2i = q img^T, t2t = q tgt^T,
    gated   S = g t2i + (1 - g) t2t (g per query)          linear  S = b1 + sum_k w1_k relu(w0_k0 t2i + w0_k1 t2t + b0_k)
    z = S / tau, loss_q2g = mean_i (lse_j z_ij - z_ii), loss_g2q = mean_j (lse_i z_ij - z_jj), loss = their mean,
    G = dL/dz = (P + Q) / (2 n) - I / n,  dL/dg_i = sum_j G_ij (t2i_ij - t2t_ij) / tau,
    dL/dw0_kc = sum_ij G_ij w1_k [pre_kij > 0] t_c,ij / tau, dL/db0_k the same without t_c, dL/dw1_k = sum_ij G_ij relu(pre_kij) / tau,
    dL/db1 = sum_ij G_ij / tau.

Budget (u = 2^-24; every bound is an fp64 tensor for `oracle.rounding.check_budget(got, ref, extra, fmt="fp32")`), built on the steps
of tests/infonce_ref.py:

1. Logits.  t2i and t2t are infonce's scores: e_t = panel_representation_bound (the three-product split) + KAPPA u (1 + 2^-7) sum |a||b|.
2. Head.  gated: fl(1 - g), two products and a sum round once each and the logit errors come in with the weights |g|, |1 - g|:
   e_s = |g| e_t2i + |1 - g| e_t2t + u (|g t2i| + 2 |(1 - g) t2t| + |s|).
   linear: relu is 1-Lipschitz, so a unit passes its pre-activation's error on: sum_k |w1_k| (|w0_k0| e_t2i + |w0_k1| e_t2t) from the
   logits, and the hidden + 2 fmas of the chain (two per pre-activation, one per unit on the running sum) cost at most (hidden + 2) u on
   the sum of the absolute terms A = |b1| + sum_k |w1_k| (|w0_k0 t2i| + |w0_k1 t2t| + |b0_k|).
3. z = fl(s fl(1 / tau)), the log-sum-exp, the loss and G exactly as infonce_ref's steps 2 - 5 with that e_s.
4. Gradients are sums over pairs of G_ij c_ij / tau with c = t2i - t2t (gated) or the unit's factor (linear).  Per term: e_G |c| +
   (|G| + e_G) e_c, e_c from step 1 (and one rounding of c); the fp32 summation: every term passes at most DEPTH additions and one
   product, (DEPTH + 1) u sum |G c| -- gated: 16 in the lane, the chunk's tiles, 8 lanes, 16 chunks; linear: 64 in the lane, 6 butterfly
   levels, the chunk's tiles, 4 waves, then fp64 -- DEPTH = 80 + ceil(n / 128) covers both; the products with fl(1 / tau) and w1_k and
   the final rounding 3 u |grad|.
   A ReLU unit whose fp64 pre-activation lies within its own error bar e_pre = |w0_k0| e_t2i + |w0_k1| e_t2t + 2 u (|w0_k0 t2i| +
   |w0_k1 t2t| + |b0_k|) may be counted on the other side: its whole contribution |G_ij| |w1_k| max(1, |t2i|, |t2t|) / tau joins the
   budgets of that unit's four gradients.

Nothing here is fitted to the device's output.  The worst measured ratios are in DESIGN.md ("Fused pair-score contrastive loss").
"""
import torch

from oracle import rounding as R

U = 2.0 ** -24
KAPPA = 10                  # tests/infonce_ref.py KAPPA
TINY = 2.0 ** -126
GATED, LINEAR = 0, 1


def _f64(x):
    return None if x is None else x.detach().double().cpu()


def _linear_parts(linear):
    w0, b0, w1, b1 = [_f64(x) for x in linear]
    return w0.reshape(-1, 2), b0.reshape(-1), w1.reshape(-1), b1.reshape(-1)[0]


def scores(mode, t2i, t2t, gate=None, linear=None):
    """S of the statement from fp64 t2i, t2t."""
    if mode == GATED:
        g = _f64(gate).reshape(-1, 1)
        return g * t2i + (1 - g) * t2t
    w0, b0, w1, b1 = _linear_parts(linear)
    s = torch.full_like(t2i, float(b1))
    for k in range(w0.shape[0]):
        s += w1[k] * torch.relu(w0[k, 0] * t2i + w0[k, 1] * t2t + b0[k])
    return s


def pairhead(mode, q, img, tgt, temperature, gate=None, linear=None):
    """fp64 statement: dict with loss, loss_q2g, loss_g2q (0-d), lse_rows, lse_cols [n], grad (gated [n]; linear [4 hidden + 1] = dw0 |
    db0 | dw1 | db1, the layout of kemr_pairhead_backward), and t2i, t2t, S, z, P, Q, G."""
    q, img, tgt = _f64(q), _f64(img), _f64(tgt)
    n = q.shape[0]
    t2i, t2t = q @ img.T, q @ tgt.T
    S = scores(mode, t2i, t2t, gate, linear)
    z = S / temperature
    lse_r, lse_c = torch.logsumexp(z, dim=1), torch.logsumexp(z, dim=0)
    diag = torch.diagonal(z)
    l_qg, l_gq = (lse_r - diag).mean(), (lse_c - diag).mean()
    P, Q = torch.exp(z - lse_r[:, None]), torch.exp(z - lse_c[None, :])
    G = (P + Q) / (2 * n) - torch.eye(n, dtype=torch.float64) / n
    Gs = G / temperature
    if mode == GATED:
        grad = (Gs * (t2i - t2t)).sum(dim=1)
    else:
        w0, b0, w1, _ = _linear_parts(linear)
        h = w0.shape[0]
        grad = torch.zeros(4 * h + 1, dtype=torch.float64)
        for k in range(h):
            pre = w0[k, 0] * t2i + w0[k, 1] * t2t + b0[k]
            gp = Gs * (pre > 0)
            grad[2 * k] = w1[k] * (gp * t2i).sum()
            grad[2 * k + 1] = w1[k] * (gp * t2t).sum()
            grad[2 * h + k] = w1[k] * gp.sum()
            grad[3 * h + k] = (Gs * torch.relu(pre)).sum()
        grad[4 * h] = Gs.sum()
    return {"loss": (l_qg + l_gq) / 2, "loss_q2g": l_qg, "loss_g2q": l_gq, "lse_rows": lse_r, "lse_cols": lse_c, "grad": grad,
            "t2i": t2i, "t2t": t2t, "S": S, "z": z, "P": P, "Q": Q, "G": G}


def split_linear_grad(grad, hidden):
    """The flat linear gradient as (dw0 [hidden, 2], db0 [hidden], dw1 [hidden], db1 [1])."""
    return grad[:2 * hidden].reshape(hidden, 2), grad[2 * hidden:3 * hidden], grad[3 * hidden:4 * hidden], grad[4 * hidden:]


def logit_bound(a, b):
    """Step 1 for one logit matrix a b^T."""
    a, b = _f64(a), _f64(b)
    _, split = R.panel_representation_bound([a], [b], 3)
    return split + KAPPA * U * (1 + 2.0 ** -7) * (a.abs() @ b.abs().T)


def softmax_budget(ref, e_z, n):
    """Steps 3 - 5 of tests/infonce_ref.py from a per-entry logit bound: (e_lse_r, e_lse_c, e_loss_q2g, e_loss_g2q, e_G)."""
    z, P, Q = ref["z"], ref["P"], ref["Q"]
    E = float(e_z.max())
    lse_fp = U * (2 * float(z.max() - z.min()) + n + 20)
    e_lse_r = E + lse_fp + 3 * U * ref["lse_rows"].abs()
    e_lse_c = E + lse_fp + 3 * U * ref["lse_cols"].abs()
    diag, e_diag = torch.diagonal(z), torch.diagonal(e_z)
    e_qg = (e_lse_r + e_diag + U * (ref["lse_rows"] - diag).abs()).mean()
    e_gq = (e_lse_c + e_diag + U * (ref["lse_cols"] - diag).abs()).mean()
    base = torch.tensor(2 * E + lse_fp + 3 * U, dtype=torch.float64)
    f_p = torch.expm1(base + 3 * U * ref["lse_rows"].abs())[:, None] + U * (2 * (z - ref["lse_rows"][:, None]).abs() + 3)
    f_q = torch.expm1(base + 3 * U * ref["lse_cols"].abs())[None, :] + U * (2 * (z - ref["lse_cols"][None, :]).abs() + 3)
    e_G = (P * f_p + Q * f_q) / (2 * n) + 3 * U * (P + Q) / (2 * n) + torch.eye(n, dtype=torch.float64) * (2 * U / n) + TINY
    return e_lse_r, e_lse_c, e_qg, e_gq, e_G


def score_bound(mode, ref, e_ti, e_tt, gate=None, linear=None):
    """Step 2: the per-entry bound of S."""
    t2i, t2t = ref["t2i"], ref["t2t"]
    if mode == GATED:
        g = _f64(gate).reshape(-1, 1)
        return g.abs() * e_ti + (1 - g).abs() * e_tt + U * ((g * t2i).abs() + 2 * ((1 - g) * t2t).abs() + ref["S"].abs())
    w0, b0, w1, b1 = _linear_parts(linear)
    h = w0.shape[0]
    carry = float((w1.abs() * w0[:, 0].abs()).sum()) * e_ti + float((w1.abs() * w0[:, 1].abs()).sum()) * e_tt
    A = torch.full_like(t2i, abs(float(b1)))
    for k in range(h):
        A += w1[k].abs() * ((w0[k, 0] * t2i).abs() + (w0[k, 1] * t2t).abs() + b0[k].abs())
    return carry + (h + 2) * U * A


def budget(mode, q, img, tgt, temperature, gate=None, linear=None, ref=None):
    """The bounds of the module docstring for one call: dict of `extra` tensors named like pairhead()'s entries."""
    q, img, tgt = _f64(q), _f64(img), _f64(tgt)
    ref = pairhead(mode, q, img, tgt, temperature, gate, linear) if ref is None else ref
    n = q.shape[0]
    t2i, t2t, z, G = ref["t2i"], ref["t2t"], ref["z"], ref["G"]
    e_ti, e_tt = logit_bound(q, img), logit_bound(q, tgt)
    e_s = score_bound(mode, ref, e_ti, e_tt, gate, linear)
    e_z = e_s / temperature + 3 * U * z.abs()
    e_lse_r, e_lse_c, e_qg, e_gq, e_G = softmax_budget(ref, e_z, n)
    Ga = G.abs() + e_G
    depth = 80 + (n + 127) // 128

    def sum_bound(c_abs, e_c):                    # a sum over pairs of G c: what G, c and the fp32 summation cost
        return e_G * c_abs + Ga * e_c + (depth + 1) * U * Ga * (c_abs + e_c)

    if mode == GATED:
        c = (t2i - t2t).abs()
        e_grad = sum_bound(c, e_ti + e_tt + U * c).sum(dim=1) / temperature + 3 * U * ref["grad"].abs()
    else:
        w0, b0, w1, _ = _linear_parts(linear)
        h = w0.shape[0]
        e_grad = torch.zeros(4 * h + 1, dtype=torch.float64)
        one, zero = torch.ones_like(t2i), torch.zeros_like(t2i)
        reach = torch.maximum(one, torch.maximum(t2i.abs(), t2t.abs()))
        for k in range(h):
            pre = w0[k, 0] * t2i + w0[k, 1] * t2t + b0[k]
            e_pre = w0[k, 0].abs() * e_ti + w0[k, 1].abs() * e_tt + 2 * U * ((w0[k, 0] * t2i).abs() + (w0[k, 1] * t2t).abs() + b0[k].abs())
            act = (pre > 0).double()
            flip = float(((pre.abs() <= e_pre) * Ga * reach).sum()) * float(w1[k].abs())
            wk = float(w1[k].abs())
            e_grad[2 * k] = wk * float(sum_bound(act * t2i.abs(), act * e_ti).sum()) + flip
            e_grad[2 * k + 1] = wk * float(sum_bound(act * t2t.abs(), act * e_tt).sum()) + flip
            e_grad[2 * h + k] = wk * float(sum_bound(act, zero).sum()) + flip
            e_grad[3 * h + k] = float(sum_bound(torch.relu(pre), act * e_pre + U * torch.relu(pre)).sum()) + flip
        e_grad[4 * h] = float(sum_bound(one, zero).sum())
        e_grad = e_grad / temperature + 3 * U * ref["grad"].abs()
    return {"loss": (e_qg + e_gq) / 2, "loss_q2g": e_qg, "loss_g2q": e_gq, "lse_rows": e_lse_r, "lse_cols": e_lse_c, "grad": e_grad,
            "S": e_s, "z": e_z}
