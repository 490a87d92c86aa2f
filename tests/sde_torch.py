"""What lt_sample_sde computes, written in torch ops on whatever device the tensors live on (helper of tests/test_sde_cpu.py and
tests/test_gpu_sde.py): one model output per stage, coefficients from a stage record of `transport.integrators.sde_table`, noise handed in.

The expressions are the tensor expressions of the host loop (integrators.py: sde, transport.py: _sde_terms / _last_step, path.py:
get_score_from_velocity) with the operands the loop has at that point: r, var, D, q as dimensioned tensors of the state dtype (the loop's
[B,1,1,1] tensors), dt / sqrt_dt / hdt as 0-dim CPU fp32 tensors, the last step's coefficients as fp32 tensors and its step size as a Python
float.  PyTorch's own type promotion and kernels then decide every rounding."""
import torch

from lumina_t2x_amd import _lib


class Stage:
    """operands of one loop stage from its record (t, r, var, D, q, dt, sqrt_dt, hdt)"""

    def __init__(self, rec, like):
        rec = [float(v) for v in rec]
        dev = lambda v: torch.tensor([v], dtype=torch.float32, device=like.device).to(like.dtype).reshape(1, 1, 1, 1)  # noqa: E731
        self.t = rec[0]
        self.r, self.var, self.D, self.q = dev(rec[1]), dev(rec[2]), dev(rec[3]), dev(rec[4])
        self.dt, self.sqrt_dt, self.hdt = (torch.tensor(v, dtype=torch.float32) for v in rec[5:8])


def drift(x, v, c):
    return v + c.D * ((c.r * v - x) / c.var)


def euler(x, v, w, c):
    dw = w * c.sqrt_dt
    mean = x + drift(x, v, c) * c.dt
    return mean + c.q * dw


def heun_xhat(x, w, c):
    dw = w * c.sqrt_dt
    return x + c.q * dw


def heun_k1(xhat, v, c):
    k1 = drift(xhat, v, c)
    return xhat + c.dt * k1, k1


def heun_out(xhat, v2, k1, xp, c2):
    return xhat + c2.hdt * (k1 + drift(xp, v2, c2))


def last(x, v, rec, rule):
    """the last-step rules at the fp32 time of the record (t, r, var, D, h, a, c, 0)"""
    rec = [float(u) for u in rec]
    f = lambda u: torch.tensor([u], dtype=torch.float32, device=x.device).reshape(1, 1, 1, 1)  # noqa: E731
    r, var, D, h = f(rec[1]), f(rec[2]), f(rec[3]), rec[4]
    score = (r * v - x) / var
    if rule == "Mean":
        return x + (v + D * score) * h
    if rule == "Tweedie":
        a = torch.tensor(rec[5], dtype=torch.float32, device=x.device)  # 0-dim, as compute_alpha_t(t)[0][0]
        c = torch.tensor(rec[6], dtype=torch.float32, device=x.device)
        return x / a + c * score
    assert rule == "Euler"
    return x + v * h


def sample(model_fn, z, noise, steps, last_rec, method, last_step):
    """the trajectory lt_sample_sde returns: the loop states and the last-step state (None without a last step).  ``model_fn(x, t)`` with
    ``t`` an fp32 [B] vector; its evaluations are counted in ``sample.nfe``"""
    B = z.shape[0]
    stages = 2 if method == "Heun" else 1
    x, xs, nfe = z, [], 0

    def model(xx, tt):
        nonlocal nfe
        nfe += 1
        return model_fn(xx, torch.full((B,), tt, dtype=torch.float32, device=z.device)).to(z.dtype)

    for i in range(noise.shape[0]):
        c = Stage(steps[i * stages], z)
        if method == "Euler":
            x = euler(x, model(x, c.t), noise[i], c)
        else:
            c2 = Stage(steps[i * stages + 1], z)
            xhat = heun_xhat(x, noise[i], c)
            xp, k1 = heun_k1(xhat, model(xhat, c.t), c)
            x = heun_out(xhat, model(xp, c2.t), k1, xp, c2)
        xs.append(x)
    fin = None
    if last_step is not None:
        fin = last(x, model(x, float(last_rec[0])), last_rec, last_step)
    sample.nfe = nfe
    return xs, fin


OPS = {"euler": _lib.LT_SDE_OP_EULER, "heun_xhat": _lib.LT_SDE_OP_HEUN_XHAT, "heun_k1": _lib.LT_SDE_OP_HEUN_K1, "heun_out": _lib.LT_SDE_OP_HEUN_OUT,
       "Mean": _lib.LT_SDE_OP_LAST_MEAN, "Tweedie": _lib.LT_SDE_OP_LAST_TWEEDIE, "Euler": _lib.LT_SDE_OP_LAST_EULER}
