"""CPU: masked (inpainting) ODE sampling - lt_sample_ode_masked / lt_sample_ode_masked_packed, transport/masked.py.  No GPU.

* the headers declare the two calls and the op entry, the library exports them and the ctypes binding has their arity;
* argument errors come back by name without a device;
* the torch expressions of the blend equal the float64 restatement of the rounding chain (tests/masked_torch.py) word for word;
* the host loop: mask = 1 everywhere is the existing fixed-grid loop, mask = 0 everywhere is the known path and ends on x1 exactly;
* ODE.sample without a mask is the function it was; the Python layer refuses masks outside [0, 1] and operands that do not broadcast."""
import ctypes as C
import re

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import masked as MK
from lumina_t2x_amd.transport.integrators import fixed_grid_odeint
from lumina_t2x_amd.transport.mini import ODE

import masked_torch as M

NEW = ("lt_sample_ode_masked", "lt_sample_ode_masked_packed", "lt_op_ode_combine_masked")


def test_headers_declare_the_calls_and_the_binding_matches():
    lib = _lib.load()
    text = _lib.header_text()
    for name in NEW:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), (name, len(args), params)
        for p, a in zip(params, args):  # pointers are pointers, floats floats, the integer widths as declared
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            elif p.startswith("float"):
                assert a is C.c_float, (name, p, a)
            elif p.startswith("int64_t"):
                assert a is C.c_int64, (name, p, a)
            else:
                assert p.startswith("int32_t") and a is C.c_int32, (name, p, a)
    # the public calls carry the triple in the order mask, source, noise, right behind the state (and the size list)
    assert re.search(r"lt_sample_ode_masked\(lt_engine\* e, const void\* z_dev, const void\* mask_dev, const void\* x1_dev, const void\* noise_dev,", text)
    assert re.search(r"lt_sample_ode_masked_packed\(lt_engine\* e, const void\* z_flat_dev, const int32_t\* hw_host, const void\* mask_flat_dev, "
                     r"const void\* x1_flat_dev,\s+const void\* noise_flat_dev,", text)


def test_argument_errors_come_back_by_name_without_a_device():
    lib = _lib.load()
    a = _lib.LtStepArgs(batch=2, io_dtype=_lib.LT_BF16)
    hw = (C.c_int32 * 4)(16, 16, 16, 16)
    grid = (C.c_float * 2)(0.0, 1.0)
    one, null = C.c_void_p(64), C.c_void_p(0)  # never dereferenced: every call below is refused before it reads anything
    for miss in range(3):
        trip = [one, one, one]
        trip[miss] = null
        assert lib.lt_sample_ode_masked(one, one, *trip, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
        assert b"lt_sample_ode_masked: null mask, source or noise" in lib.lt_last_error()
        assert lib.lt_sample_ode_masked_packed(one, one, hw, *trip, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
        assert b"lt_sample_ode_masked_packed: null mask, source or noise" in lib.lt_last_error()
        assert lib.lt_op_ode_combine_masked(0, one, one, None, None, None, *trip, one, 1, 0.25, 0.5, 0.5, 16, None) != 0
        assert b"ode_combine_masked: null mask, source or noise" in lib.lt_last_error()
    assert lib.lt_sample_ode_masked(None, one, one, one, one, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_masked: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_masked(one, one, one, one, one, None, one, None, 2, 0, 1, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_masked: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_masked_packed(None, one, hw, one, one, one, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_masked_packed: null argument" in lib.lt_last_error()
    assert lib.lt_sample_ode_masked_packed(one, one, None, one, one, one, None, one, grid, 2, 0, 1, 1, C.byref(a), None) != 0
    assert b"lt_sample_ode_masked_packed: null argument" in lib.lt_last_error()
    for mode in (1, 2, 3, 5, -1):  # the stage-internal combines are not blended: no such mode
        assert lib.lt_op_ode_combine_masked(mode, one, one, one, one, one, one, one, one, one, 1, 0.25, 0.5, 0.5, 16, None) != 0
        assert b"ode_combine_masked: bad mode" in lib.lt_last_error()
    assert lib.lt_op_ode_combine_masked(0, one, one, None, None, None, one, one, one, one, 2, 0.25, 0.5, 0.5, 16, None) != 0
    assert b"state dtype" in lib.lt_last_error()
    assert lib.lt_op_ode_combine_masked(4, one, one, one, None, one, one, one, one, one, 1, 0.25, 0.5, 0.5, 16, None) != 0
    assert b"null state or slope" in lib.lt_last_error()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mask_kind", ["hard", "eighths", "ones", "zeros"])
def test_torch_expressions_equal_the_float64_restatement_word_for_word(dtype, mask_kind):
    for t in M.T_VALUES:
        step, m, noise, x1 = M.operands(4097, dtype, 3, mask_kind)
        got = M.blend(step, m, noise, x1, t)
        want = M.chain64(step, m, noise, x1, t, dtype)
        assert got.dtype == dtype and bool(torch.isfinite(got.float()).all())
        assert torch.equal(M.bits(got), M.bits(want)), (t, int((M.bits(got) != M.bits(want)).sum()))
        # the package's own text is the same text
        assert torch.equal(M.bits(MK.blend(step, m, noise, x1, t)), M.bits(got))
        assert torch.equal(M.bits(MK.known(noise, x1, t)), M.bits(M.known(noise, x1, t)))


def test_the_scalars_of_the_known_path_multiply_in_fp32_and_are_not_rounded_to_the_state_dtype():
    """what the kernel's fp32 scalar arguments rest on: t and 1 - t enter the bf16 products un-rounded (1 - t formed in double first)"""
    _, _, noise, x1 = M.operands(4097, torch.bfloat16, 5, "hard")
    t = 0.7283
    got = M.known(noise, x1, t)
    tb, ob = float(torch.tensor(t).to(torch.bfloat16)), float(torch.tensor(1 - t).to(torch.bfloat16))
    cast_first = (noise.float() * ob).to(torch.bfloat16) + (x1.float() * tb).to(torch.bfloat16)
    assert not torch.equal(got, cast_first)
    in_fp32 = (noise.float() * float(torch.tensor(1 - t, dtype=torch.float32))).to(torch.bfloat16) + (x1.float() * float(torch.tensor(t))).to(torch.bfloat16)
    assert torch.equal(M.bits(got), M.bits(in_fp32))


def _toy(y, tvec, gain=1.0):
    """a drift with state and time in it, cheap and deterministic"""
    return (torch.sin(y.float() * 1.7) * gain + tvec.float().view(-1, 1, 1, 1) - 0.3 * y.float()).to(y.dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_host_loop_limits_all_ones_and_all_zeros(dtype, method):
    g = torch.Generator().manual_seed(1)
    z, x1, noise = (torch.randn(2, 4, 6, 10, generator=g).to(dtype) for _ in range(3))
    tgrid = torch.linspace(0.0, 1.0, 6)
    tgrid = tgrid / (tgrid + 4 - 4 * tgrid)

    def fn(t, y):  # as mini.ODE.sample forms it
        return _toy(y, torch.ones(y.size(0)) * t, gain=0.8)

    plain = fixed_grid_odeint(fn, z, tgrid, method=method)
    ones = MK.sample_masked(_toy, z, tgrid, torch.ones_like(z), x1, noise, method, gain=0.8)
    assert ones.dtype == dtype and torch.equal(ones, plain)
    zeros = MK.sample_masked(_toy, z, tgrid, torch.zeros_like(z), x1, noise, method, gain=0.8)
    assert torch.equal(zeros[0], z)
    for i in range(1, len(tgrid)):
        assert torch.equal(zeros[i], MK.known(noise, x1, float(tgrid[i]))), i
    assert torch.equal(M.bits(zeros[-1]), M.bits(x1))
    # a hard mask: kept pixels lie on the known path at every grid point, the others moved away from it
    m = torch.zeros_like(z)
    m[..., 2:5, 3:8] = 1
    mixed = MK.sample_masked(_toy, z, tgrid, m, x1, noise, method, gain=0.8)
    for i in range(1, len(tgrid)):
        k = MK.known(noise, x1, float(tgrid[i]))
        assert torch.equal(mixed[i][m == 0], k[m == 0]) and not torch.equal(mixed[i][m == 1], k[m == 1]), i


def test_ode_sample_without_a_mask_is_the_function_it_was_and_routes_a_mask_to_the_host_loop():
    g = torch.Generator().manual_seed(2)
    z, x1, noise = (torch.randn(2, 4, 8, 8, generator=g) for _ in range(3))
    o = ODE(9, "midpoint", 4, strength=0.6)

    def fn(t, y):
        return _toy(y, torch.ones(y.size(0)) * t)

    want = fixed_grid_odeint(fn, z, o.t, method="midpoint")
    assert torch.equal(o.sample(z, _toy), want) and torch.equal(o.sample(z, _toy, mask=None, x1=None, noise=None), want)
    m = torch.zeros(8, 8)
    m[2:6, 1:5] = 0.5
    got = o.sample(z, _toy, mask=m, x1=x1[:1], noise=noise[:1], gain=1.0)
    em, ex, en = MK.expand_operands(z, m, x1[:1], noise[:1])
    assert em.shape == z.shape and torch.equal(em[1, 3], m) and torch.equal(ex[1], x1[0]) and torch.equal(en[0], noise[0])
    assert torch.equal(got, MK.sample_masked(_toy, z, o.t, em, ex, en, "midpoint"))
    assert got.shape == (len(o.t),) + tuple(z.shape) and torch.equal(got[-1][em == 0], ex[em == 0])
    with pytest.raises(ValueError, match="together"):
        o.sample(z, _toy, mask=m)
    with pytest.raises(NotImplementedError, match="fixed-grid"):
        ODE(5, "dopri5").sample(z, _toy, mask=m, x1=x1, noise=noise)


def test_the_python_layer_refuses_bad_masks_and_operands_that_do_not_broadcast():
    z = torch.zeros(4, 4, 8, 12, dtype=torch.bfloat16)
    x1, noise = torch.zeros(1, 4, 8, 12), torch.zeros(2, 4, 8, 12)
    ok = torch.rand(8, 12)
    m, s, n = MK.expand_operands(z, ok, x1, noise)  # [H, W]; one source for all rows; two noises repeated for the uncond half
    assert all(v.shape == z.shape and v.dtype == z.dtype and v.is_contiguous() for v in (m, s, n))
    assert torch.equal(m[3, 2], ok.to(torch.bfloat16))  # rounded to the state dtype, once
    for bad in (ok + 0.5, ok - 0.5, torch.full((8, 12), float("nan")), torch.full((8, 12), 1.0009765625)):
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            MK.expand_operands(z, bad, x1, noise)
    with pytest.raises(ValueError, match="floating-point"):
        MK.expand_operands(z, torch.ones(8, 12, dtype=torch.bool), x1, noise)
    for shape in ((8, 10), (3, 1, 8, 12), (1, 1, 1, 8, 12), (4, 8)):
        with pytest.raises(ValueError, match="mask"):
            MK.expand_operands(z, torch.ones(shape), x1, noise)
    with pytest.raises(ValueError, match="x1"):
        MK.expand_operands(z, ok, torch.zeros(3, 4, 8, 12), noise)
    with pytest.raises(ValueError, match="noise"):
        MK.expand_operands(z, ok, x1, torch.zeros(1, 3, 8, 12))
    # the list form
    zs = [torch.zeros(4, 8, 12), torch.zeros(4, 6, 6)] * 2
    ms, ss, ns = MK.expand_operands_packed(zs, [torch.ones(8, 12), torch.zeros(1, 6, 6)], [z_.clone() for z_ in zs], [z_.clone() for z_ in zs[:2]])
    assert [tuple(v.shape) for v in ms] == [tuple(v.shape) for v in zs] == [tuple(v.shape) for v in ns]
    with pytest.raises(ValueError, match="entries"):
        MK.expand_operands_packed(zs, [torch.ones(8, 12)], zs, zs)
    with pytest.raises(ValueError, match=r"mask\[1\]"):
        MK.expand_operands_packed(zs, [torch.ones(8, 12), torch.ones(8, 12)], zs, zs)
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        MK.expand_operands_packed(zs, [torch.ones(8, 12), torch.full((6, 6), 2.0)], zs, zs)
    with pytest.raises(ValueError, match="shape and dtype"):
        MK.sample_masked(_toy, z, [0.0, 1.0], ok, z, z)


def test_driver_mask_goes_to_the_latent_grid_by_area_and_the_threshold_binarises_it():
    from lumina_t2x_amd import sample_img2img as S
    pix = torch.zeros(32, 48)
    pix[:16, :20] = 1.0  # columns 16..19 cover half of the third latent column
    soft = S.latent_mask(pix, 4, 6)
    assert soft.shape == (1, 1, 4, 6) and soft.dtype == torch.float32
    want = torch.zeros(4, 6)
    want[:2, :2] = 1.0
    want[:2, 2] = 0.5
    assert torch.equal(soft[0, 0], want)
    assert torch.equal(S.latent_mask(pix, 4, 6, 0.4)[0, 0], (want > 0.4).float()) and torch.equal(S.latent_mask(pix, 4, 6, 0.5)[0, 0], (want > 0.5).float())
    args = S.build_parser().parse_args(["--ckpt", "x", "--image", "y"])
    assert args.mask == "" and args.mask_threshold is None
