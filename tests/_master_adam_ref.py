"""The master-weight Adam step restated in plain torch on the CPU (test-only): torch.optim.Adam over fp32 tensors fed
the bf16 gradient, then the bf16 parameter as the rounded master.  cc_adam_master_step is checked against it, and the
host tests use it to show what the bf16-state optimizer cannot do."""
import torch


class MasterAdamRef:
    """fp32 masters `p32` (and torch's fp32 moments) of one flat parameter; step(g16, coef) applies
    torch.optim.Adam(foreach=False) with grad = g16.float() * coef and returns the bf16 parameter p32.to(bfloat16)."""

    def __init__(self, p32, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, exp_avg=None, exp_avg_sq=None, step=0):
        self.p32 = torch.nn.Parameter(p32.detach().clone().float().cpu())
        self.opt = torch.optim.Adam([self.p32], lr=lr, betas=betas, eps=eps, foreach=False)
        if exp_avg is not None or step:
            self.opt.state[self.p32] = {
                "step": torch.tensor(float(step)),
                "exp_avg": (exp_avg if exp_avg is not None else torch.zeros_like(self.p32)).detach().clone().float(),
                "exp_avg_sq": (exp_avg_sq if exp_avg_sq is not None
                               else torch.zeros_like(self.p32)).detach().clone().float()}

    def step(self, g16, coef=1.0):
        assert g16.dtype == torch.bfloat16
        self.p32.grad = g16.detach().float().cpu() * float(torch.tensor(coef, dtype=torch.float32))
        self.opt.step()
        return self.p16

    @property
    def p16(self):
        return self.p32.detach().to(torch.bfloat16)

    @property
    def exp_avg(self):
        return self.opt.state[self.p32]["exp_avg"]

    @property
    def exp_avg_sq(self):
        return self.opt.state[self.p32]["exp_avg_sq"]


def bf16_adam_step(p, g, m, v, step, lr=5e-5, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam step with bf16 parameter and moments (the default mode's arithmetic: every torch op's
    result rounded to bf16), in place."""
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / ((1 - beta2 ** step) ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1 - beta1 ** step))
