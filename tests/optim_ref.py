"""TEST INFRASTRUCTURE ONLY — plain float64 references for the optimizer kernels of espresso_amd/csrc/optim.hip, on the fp32
operands the kernels receive (every scalar argument is first rounded to fp32, as the C ABI does).

sumsq       sum g^2
clip_coef   coef[0] = scale * min(1, max_norm / (norm + 1e-6)), coef[1] = norm = sqrt(sumsq) * scale, scale = pre_scale [/ denom];
            a non-finite norm gives a non-finite coef[0]
step_size   lr * sqrt(1 - beta2^t) / (1 - beta1^t) in double, as ea_adam_step computes it (the kernel then rounds it to fp32)
adam_step   fairseq's form (fairseq/optim/adam.py:215-240): m = beta1 m + (1 - beta1) g', v = beta2 v + (1 - beta2) g'^2,
            denom = sqrt(v) + eps, decoupled weight decay p += p * (-wd * lr), then p += -step_size * m / denom; with the bounds of
            tests/test_optimizer_kernels.py's docstring, and one deliberate defect (`mut`) for the mutation tests"""
import math

import torch

E23 = 2.0 ** -23
F64 = torch.float64
MUTATIONS = ("betas_swapped", "eps_inside_sqrt", "decay_after_update", "clip_dropped", "bias_correction_of_t_minus_1", "tail_element_skipped")


def f32(x):
    """a Python float as the fp32 value the C ABI passes"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def sumsq(g, prefill=0.0):
    g = g.double()
    return float(prefill) + float((g * g).sum())


def clip_coef(ss, pre_scale, denom, max_norm):
    """ss, denom: the fp32 device scalars as Python floats (denom None: not given) -> (coef0, coef1)"""
    t = lambda x: torch.tensor(float(x), dtype=F64)
    ps = t(f32(pre_scale))
    if denom is not None:
        ps = ps / t(denom)
    norm = float(torch.sqrt(t(ss)) * ps)
    ps = float(ps)
    if not math.isfinite(norm):
        return float(t(ps) * t(norm)), norm
    c = 1.0
    if f32(max_norm) > 0:
        c = min(1.0, f32(max_norm) / (norm + f32(1e-6)))
    return ps * c, norm


def step_size(lr, beta1, beta2, t):
    return f32(lr) * math.sqrt(1.0 - f32(beta2) ** t) / (1.0 - f32(beta1) ** t)


def adam_step(p, g, m, v, gs, lr, beta1, beta2, eps, wd, t, mut=None):
    """p, g, m, v: fp32 tensors; gs: the gradient scale (coef[0], or 1.0 without coef) -> dict of float64 tensors p, m, v and their
    bounds tp, tm, tv.  A non-finite gs is the skip path: the operands unchanged, bounds 0."""
    assert mut is None or mut in MUTATIONS
    p0, g0, m0, v0 = p.double(), g.double(), m.double(), v.double()
    if not math.isfinite(gs):
        z = torch.zeros_like(p0)
        return {"p": p0, "m": m0, "v": v0, "tp": z, "tm": z, "tv": z}
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    if mut == "betas_swapped":
        b1, b2 = b2, b1
    if mut == "clip_dropped":
        gs = 1.0
    ss = step_size(lr, beta1, beta2, t - 1 if mut == "bias_correction_of_t_minus_1" else t)
    gg = g0 * gs
    a1, a2 = m0 * b1, (1.0 - b1) * gg
    mm = a1 + a2
    c1, c2 = v0 * b2, (1.0 - b2) * gg * gg
    vv = c1 + c2
    den = torch.sqrt(vv + eps) if mut == "eps_inside_sqrt" else torch.sqrt(vv) + eps
    q = mm / den
    upd = -ss * q
    dec = p0 * (-wd * lr)
    if mut == "decay_after_update":
        p1 = p0 + upd
        pp = p1 + p1 * (-wd * lr)
    else:
        p1 = p0 + dec if wd != 0 else p0
        pp = p1 + upd
    if mut == "tail_element_skipped":
        for new, old in ((pp, p0), (mm, m0), (vv, v0)):
            new[-1] = old[-1]
    # bounds: E23 per fp32 rounding (optim.hip:71-76)
    tm = 3 * E23 * (a1.abs() + a2.abs())                         # g gs, m beta1, (1 - beta1) gg, the addition
    tv = 6 * E23 * (c1 + c2)                                     # gg twice (2), two products, v beta2, the addition
    sq = torch.sqrt(vv)
    tden = torch.where(vv > 0, tv / (2 * sq.clamp_min(1e-300)), torch.zeros_like(vv)) + E23 * sq + E23 * den   # sqrtf, + eps
    tq = tm / den + mm.abs() * tden / (den * den) + E23 * q.abs()                                           # the division
    tupd = abs(ss) * tq + 2 * E23 * upd.abs()                    # step_size's own rounding to fp32, the product
    tp1 = (2 * E23 * dec.abs() + E23 * p1.abs()) if wd != 0 else torch.zeros_like(p0)   # -wd lr, the product, the addition
    tp = tp1 + tupd + E23 * pp.abs()
    return {"p": pp, "m": mm, "v": vv, "tp": tp, "tm": tm, "tv": tv}


def bf16_rne(x):
    """fp32 tensor -> the bf16 round-to-nearest-even of it (torch's own conversion)"""
    return x.float().to(torch.bfloat16)
