"""Phase Upscale of the reference's visual_anagrams/generate.py:465-494 restated in torch, rounding point by rounding point - shared by
tests/test_views_upscale_cpu.py, tests/test_gpu_views_upscale.py and scripts/make_views_upscale_golden.py.  TEST INFRASTRUCTURE ONLY.

Two statements of the same loop:
  ``chain_loop``       the chain the kernels implement (csrc/views.hip): fp32 arithmetic with an explicit rounding R to the state dtype after
                       every product and sum, the four coefficients taken from ``transport.integrators.views_guided_table``
  ``expression_loop``  the reference's tensor expressions (generate.py:232-262, :486-494) typed out on tensors of the state dtype, with the views
                       applied through view objects; the decay factor ``c`` is the 0-dim fp32 CPU tensor the reference builds, or (``c_as="float"``)
                       its value as a Python float, which multiplies a tensor of any dtype in fp32 on every device
Both take ``fwd(x [V, C, H, W], t float, stage index) -> [V, C, H, W]``: the model outputs of all views at one stage, however they are made
(one batched evaluation, one evaluation per view, or outputs stored in a fixture).
"""
import torch

from lumina_t2x_amd.transport.integrators import views_guided_table


def rounder(dtype):
    return (lambda x: x) if dtype == torch.float32 else (lambda x: x.to(dtype).float())


def chain_input(y, G, Z, f0, half_dt, coef, views, dtype):
    """the model inputs [V, C, H, W] of one stage (views.hip: views_guided_gather_kernel); y, G, Z [C, H, W] and f0 [V, C, H, W] (None at stage 0)
    hold state-dtype values; coef = (ft, f1t, kc, k1c) fp32 tensors / floats"""
    R = rounder(dtype)
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32)
    ft, f1t, kc, k1c = (f32(v) for v in coef)
    y, G, Z = y.float(), G.float(), Z.float()
    g = R(R(ft * G) + R(f1t * Z))
    out = []
    for v, vw in enumerate(views):
        s = y if f0 is None else R(y + vw.inverse_view(R(f0[v].float() * f32(half_dt))))
        out.append(vw.view(R(R(k1c * s) + R(kc * g))))
    return torch.stack(out).to(dtype)


def chain_close(y, f1, dt, views, dtype):
    """y' = R(y - R(sum_v inverse_view_v(-R(f1_v * dt)) / V)), fp32 sum in view order (views.hip: views_reduce_kernel)"""
    R = rounder(dtype)
    acc = torch.zeros_like(y, dtype=torch.float32)
    for v, vw in enumerate(views):
        acc = acc + vw.inverse_view(-R(f1[v].float() * torch.tensor(dt, dtype=torch.float32)))
    # (a tensor divisor: by a Python scalar torch's device kernels multiply with the reciprocal, which is not the division for V = 3)
    return R(y.float() - R(acc / torch.full_like(acc, float(len(views))))).to(dtype)


def chain_loop(fwd, views, z, guidance, noise, grid, coef_rounding, record=None):
    """z, guidance, noise [1, C, H, W] of the state dtype; grid: Python floats.  Returns the states [n, C, H, W].  ``record``: a list that
    receives every stage's model input"""
    dtype = z.dtype
    coef = views_guided_table(grid, dtype, coef_rounding)
    y, G, Z = z[0].clone(), guidance[0], noise[0]
    states = [y.clone()]
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        x0 = chain_input(y, G, Z, None, 0.0, coef[i, 0], views, dtype)
        f0 = fwd(x0, t0, 2 * i)
        x1 = chain_input(y, G, Z, f0, half_dt, coef[i, 1], views, dtype)
        f1 = fwd(x1, t0 + half_dt, 2 * i + 1)
        if record is not None:
            record += [x0, x1]
        y = chain_close(y, f1, dt, views, dtype)
        states.append(y.clone())
    return torch.stack(states)


def expression_scalars(t, c_as="tensor"):
    """(t, 1 - t, c, 1 - c) of generate.py:239-241: Python floats and the 0-dim fp32 CPU tensor c ("tensor": as the reference has them), or all
    four as Python floats holding the fp32 values ("float": PyTorch multiplies a tensor of any dtype by a Python float in fp32)"""
    c = 0.5 * (1 + torch.cos(torch.pi * torch.tensor(t))).cpu()  # decay factor
    if c_as == "float":
        return float(torch.tensor(t, dtype=torch.float32)), float(torch.tensor(1 - t, dtype=torch.float32)), c.item(), (1 - c).item()
    return t, 1 - t, c, 1 - c


def expression_input(y0, guidance, noise, f0, half_dt, scalars, views):
    """generate.py:240-258 for every view: y0, guidance, noise [C, H, W] tensors of the state dtype on one device; f0 [V, C, H, W] or None;
    scalars = (t, 1 - t, c, 1 - c)"""
    a, b, c, c1 = scalars
    guidance_t = a * guidance + b * noise  # (/ anchor: all ones)
    out = []
    for v, vw in enumerate(views):
        y = y0
        if f0 is not None:
            noise_pred = -f0[v] * half_dt
            y = y0 - vw.inverse_view(noise_pred)
        out.append(vw.view(c1 * y + c * guidance_t))
    return torch.stack(out)


def expression_loop(fwd, views, z, guidance, noise, grid, c_as="tensor", record=None, close=None):
    """generate.py:465-494 with ``midpoint_solver_extra`` typed out; tensors of the state dtype on z's device.  ``close(y, f1, dt)``: another
    statement of the closing update (default: the reference's stack(...).mean(0) form)"""
    y, G, Z = z[0].clone(), guidance[0], noise[0]
    states = [y.clone()]
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = t1 - t0
        half_dt = 0.5 * dt
        x0 = expression_input(y, G, Z, None, half_dt, expression_scalars(t0, c_as), views)
        f0 = fwd(x0, t0, 2 * i)
        x1 = expression_input(y, G, Z, f0, half_dt, expression_scalars(t0 + half_dt, c_as), views)
        f1 = fwd(x1, t0 + half_dt, 2 * i + 1)
        if record is not None:
            record += [x0, x1]
        if close is not None:
            y = close(y, f1, dt)
        else:
            inverted = [vw.inverse_view(-(f1[v] * dt)) for v, vw in enumerate(views)]
            y = y - torch.stack(inverted).mean(dim=0)
        states.append(y.clone())
    return torch.stack(states)


def chunks_cover(seqlen, base_seqlen):
    """visual_anagrams/models/nextdit.py:336-352 on integers: do int(seqlen / base_seqlen + 0.99) chunks of base_seqlen rows reach the last row"""
    return int(seqlen / base_seqlen + 0.99) * base_seqlen >= seqlen
