"""Pure-torch CPU reference of the JumpReLU crosscoder: the mask, gate and window from the
bit rules, the threshold gradient in fp64, the clip finaliser's arithmetic, and a whole reference training step
(autograd with the JumpReLU and Heaviside straight-through estimators, torch's clip_grad_norm_ over the five
parameters, torch's Adam)."""
import torch

from oracle import cpu_reference as O

BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
PARAMS5 = tuple(O.PARAM_ORDER) + ("jump_threshold",)


def positive_on_bits(a):
    """a > 0 on the element's bits: sign clear, not zero, not NaN; +inf and subnormals count."""
    inf = 0x7F80 if a.dtype == torch.bfloat16 else 0x7F800000
    mask = 0xFFFF if a.dtype == torch.bfloat16 else 0xFFFFFFFF
    u = a.contiguous().view(BITS[a.dtype]).to(torch.int64) & mask
    return (u >= 1) & (u <= inf)


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def jumprelu_ref(a, theta, eps):
    """a [B, h] (bf16 or fp32, = relu(pre) as G1 rounds it), theta fp32 [h], eps a float (taken in fp32).
    kept: a > 0 on its bits and float(a) > theta; gated: a > 0 and d > -half; window: a > 0 and -half < d < half,
    with d = float(a) - theta one fp32 subtract and half = 0.5f * eps.  dense / gate: the bits kept, else +0."""
    assert theta.dtype == torch.float32
    pos = positive_on_bits(a)
    af, th = a.float(), theta[None, :]
    half = f32(0.5) * f32(eps)
    d = af - th
    kept = pos & (af > th)
    gated = pos & (d > -half)
    window = gated & (d < half)
    zero = torch.zeros_like(a)
    return {"kept": kept, "gated": gated, "window": window, "dense": torch.where(kept, a, zero),
            "gate": torch.where(gated, a, zero), "count": kept.sum(1), "d": d}


def theta_grad_terms(G, window, theta, eps, l0_scale):
    """fp64 [B, h]: window * (-(theta / eps) G - l0_scale / eps), eps and l0_scale taken as the fp32 values the kernel
    is handed; their column sums are theta.grad."""
    e, s = f32(eps).double(), f32(l0_scale).double()
    t = -(theta.double()[None, :] / e) * G.double() - s / e
    return torch.where(window, t, torch.zeros_like(t))


def bwd_ref(g_pre, ref):
    """g_pre after cc_jumprelu_bwd: +0 where gated but not kept, untouched elsewhere."""
    return torch.where(ref["gated"] & ~ref["kept"], torch.zeros_like(g_pre), g_pre)


# ----------------------------------------------------------------------------- the clip finaliser's arithmetic
def bf16r(v):
    return v.to(torch.bfloat16).to(torch.float32)


def clip_param_norms(sq_sums, emulate=0):
    """grad_tail.h's clip_param_norm from the per-parameter squared sums (python floats / fp64), fp32 values.
    emulate 0: fp32 gradients; 1: bf16 gradients; 2: four bf16 gradients followed by fp32 ones."""
    norms = []
    for p, s in enumerate(sq_sums):
        nr = torch.tensor(float(s), dtype=torch.float64).sqrt().to(torch.float32)
        norms.append(bf16r(nr) if emulate == 1 or (emulate == 2 and p < 4) else nr)
    return norms


def clip_from_norms(norms, max_norm=1.0, emulate=0):
    """grad_tail.h's clip_coef from the per-parameter norms (fp32 values): (coef, total) as fp32 tensors."""
    norms = list(norms)
    if emulate == 2:  # torch stacks the dtype groups of that list with the fp32 group first
        norms = norms[4:] + norms[:4]
    s = f32(0.0)
    for nr in norms:
        s = s + nr.float() * nr.float()
    total = s.sqrt()
    if emulate == 1:
        total = bf16r(total)
        den = bf16r(total + f32(1e-6))
        return torch.minimum(bf16r(f32(max_norm) / den), f32(1.0)), total
    return torch.minimum(f32(max_norm) / (total + f32(1e-6)), f32(1.0)), total


def clip_finaliser(sq_sums, max_norm=1.0, emulate=0):
    """grad_tail.h's clip_finish: (coef, total, norms)."""
    norms = clip_param_norms(sq_sums, emulate)
    coef, total = clip_from_norms(norms, max_norm, emulate)
    return coef, total, torch.stack(norms)


# ----------------------------------------------------------------------------- the straight-through estimators
class JumpReLUSTE(torch.autograd.Function):
    """a * H(a - theta).  d/da: the straight-through gradient at the kept elements; d/dtheta:
    sum_b window * (-(theta / eps)) * g (Rajamanoharan et al. 2024, the rectangle kernel)."""

    @staticmethod
    def forward(ctx, a, theta, kept, window, eps):
        ctx.save_for_backward(theta, kept, window)
        ctx.eps = eps
        return a * kept.to(a.dtype)

    @staticmethod
    def backward(ctx, g):
        theta, kept, window = ctx.saved_tensors
        g_theta = (-(theta[None, :] / ctx.eps) * g.to(theta.dtype) * window.to(theta.dtype)).sum(0)
        return g * kept.to(g.dtype), g_theta, None, None, None


class HeavisideSTE(torch.autograd.Function):
    """H(a - theta), fp32 / theta's dtype.  d/da: none; d/dtheta: sum_b window * (-1 / eps) * g."""

    @staticmethod
    def forward(ctx, a, theta, kept, window, eps):
        ctx.save_for_backward(window)
        ctx.eps = eps
        return kept.to(theta.dtype)

    @staticmethod
    def backward(ctx, g):
        window, = ctx.saved_tensors
        return None, (-(1.0 / ctx.eps) * g * window.to(g.dtype)).sum(0), None, None, None


def jr_losses(x, P, theta, eps, dtype, A=None, masks=None):
    """oracle.get_losses (crosscoder.py:96-130) of a JumpReLU crosscoder: x [B, n, d], P the four reference
    parameters in `dtype`, theta [h] (fp32, or fp64 in the fp64 evaluation).  A (optional, [B, h]): activations
    imposed on relu(pre) -- their values, the CPU graph's gradient -- so that only arithmetic differs from the
    run that produced them.  masks: jumprelu_ref's of the activations (default: computed from them in fp32; the
    window is restricted to a > 0).  Returns the loss dict, with "acts"."""
    x = x.to(dtype)
    a = O.encode(x, P)
    if A is not None:
        a = a + (A.to(dtype) - a).detach()
    if masks is None:
        src = A if A is not None else a.detach()
        masks = jumprelu_ref(src if src.dtype in BITS else src.float(), theta.detach().float(), eps)
    kept, window = masks["kept"], masks["window"]
    e = float(f32(eps)) if theta.dtype != torch.float64 else float(f32(eps).double())
    acts = JumpReLUSTE.apply(a, theta, kept, window, e)
    l0 = HeavisideSTE.apply(a, theta, kept, window, e).sum(-1).mean()
    recon = O.decode(acts, P)
    diff = recon.float() - x.float() if dtype != torch.float64 else recon - x
    l2_per_batch = diff.pow(2).sum(dim=(1, 2))
    total_variance = (x - x.mean(0)).pow(2).sum(dim=(1, 2))
    ev = 1 - l2_per_batch / (total_variance + 1e-8)
    ev_m = []
    for m in (0, 1):
        per_tok = (recon[:, m, :] - x[:, m, :]).pow(2).sum(dim=-1).squeeze()
        tv = (x[:, m, :] - x[:, m, :].mean(0)).pow(2).sum(-1).squeeze()
        ev_m.append(1 - per_tok / (tv + 1e-8))
    total_decoder_norm = P["W_dec"].norm(dim=-1).sum(dim=1)
    return {"l2_loss": l2_per_batch.mean(), "l1_loss": (acts * total_decoder_norm[None, :]).sum(-1).mean(0),
            "l0_loss": l0, "explained_variance": ev, "explained_variance_A": ev_m[0],
            "explained_variance_B": ev_m[1], "recon": recon, "acts": acts}


def jr_loss_and_grads(x, P, theta, eps, dtype, l1c, l0c, A=None):
    """autograd of l2 + l1c l1 + l0c l0 on leaf copies: (loss dict, objective, the five gradients)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    th = theta.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)
    lo = jr_losses(x, leaves, th, eps, dtype, A=A)
    loss = lo["l2_loss"] + l1c * lo["l1_loss"] + l0c * lo["l0_loss"]
    loss.backward()
    grads = {k: leaves[k].grad for k in O.PARAM_ORDER}
    grads["jump_threshold"] = th.grad if th.grad is not None else torch.zeros_like(th)
    return lo, loss, grads


class JumpReLUOracleTrainer:
    """Trainer.step of a JumpReLU crosscoder restated on the CPU: the objective above with l1_coeff and l0_coeff on
    the reference's warm-up schedule, torch.nn.utils.clip_grad_norm_(max_norm=1.0) over the five parameters (the
    thresholds fp32 in every mode) and torch.optim.Adam."""

    def __init__(self, cfg, P, theta):
        self.cfg = cfg
        self.dtype = O.DTYPES[cfg["enc_dtype"]]
        self.eps = cfg.get("jump_bandwidth", 1e-3)
        self.P = {k: torch.nn.Parameter(v.detach().to(self.dtype).clone()) for k, v in P.items()}
        self.P["jump_threshold"] = torch.nn.Parameter(theta.detach().float().clone())
        self.total_steps = cfg["num_tokens"] // cfg["batch_size"]
        self.step_counter = 0
        self.opt = torch.optim.Adam([self.P[k] for k in PARAMS5], lr=cfg["lr"], betas=(cfg["beta1"], cfg["beta2"]),
                                    foreach=False)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda s: O.lr_lambda(s, self.total_steps))
        self.last_total_norm = None

    def step(self, x, A=None):
        l1c = O.l1_coeff(self.step_counter, self.total_steps, self.cfg["l1_coeff"])
        l0c = O.l1_coeff(self.step_counter, self.total_steps, self.cfg["l0_coeff"])
        four = {k: self.P[k] for k in O.PARAM_ORDER}
        lo = jr_losses(x, four, self.P["jump_threshold"], self.eps, self.dtype, A=A)
        base = lo["l2_loss"] + l1c * lo["l1_loss"]
        loss = base + l0c * lo["l0_loss"]
        self.opt.zero_grad()
        loss.backward()
        if self.P["jump_threshold"].grad is None:
            self.P["jump_threshold"].grad = torch.zeros_like(self.P["jump_threshold"])
        self.last_total_norm = torch.nn.utils.clip_grad_norm_([self.P[k] for k in PARAMS5], max_norm=1.0)
        self.opt.step()
        self.sched.step()
        d = {"loss": loss.item(), "l2_loss": lo["l2_loss"].item(), "l1_loss": lo["l1_loss"].item(),
             "l0_loss": lo["l0_loss"].item(), "l1_coeff": l1c, "lr": self.sched.get_last_lr()[0],
             "explained_variance": lo["explained_variance"].mean().item(),
             "explained_variance_A": lo["explained_variance_A"].mean().item(),
             "explained_variance_B": lo["explained_variance_B"].mean().item(), "l0_coeff": l0c}
        self.step_counter += 1
        return d

    def moments(self, key):
        st = self.opt.state[self.P[key]]
        return st["exp_avg"], st["exp_avg_sq"]
