"""CPU: smoothed-energy guidance - seg_taps, the float64 blur restatement against the dense blur matrix, the table / layer-set checks,
every refuse_with_seg message, and the host loop sample_cfg_seg on a stub model."""
import ctypes as C
import math

import pytest
import torch

import lumina_t2x_amd  # noqa: F401
from lumina_t2x_amd import _lib
from lumina_t2x_amd.transport import guidance as G
from lumina_t2x_amd.transport.mini import ODE

import exact_seg as XS


def test_seg_taps_sum_symmetry_radius_and_inf():
    for sigma in (0.05, 0.3, 1.0, 2.5, 10.0, 10.2, 40.0):
        mode, r, taps = G.seg_taps(sigma)
        assert mode == 0 and r == min(math.ceil(3 * float(torch.tensor(sigma, dtype=torch.float32))), 31) and r <= G.SEG_MAX_RADIUS
        assert taps.dtype == torch.float32 and taps.numel() == 2 * r + 1
        assert torch.equal(taps, taps.flip(0))
        assert abs(float(taps.double().sum()) - 1.0) <= (2 * r + 1) * 2.0 ** -25
        assert bool((taps[:r + 1].diff() >= 0).all()) and float(taps[r]) == float(taps.max())
    assert G.seg_taps(10.0)[1] == 30 and G.seg_taps(40.0)[1] == 31
    mode, r, taps = G.seg_taps(math.inf)
    assert (mode, r, taps.numel()) == (1, 0, 0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="not positive"):
            G.seg_taps(bad)


def test_the_engine_derives_the_same_taps_word_for_word():
    L = _lib.load()
    buf, r, mode = (C.c_float * 63)(), C.c_int32(), C.c_int32()
    for sigma in (0.05, 0.3, 1.0, 2.5, 7.77, 10.0, 10.2, 40.0, math.inf):
        assert L.lt_op_seg_taps(sigma, buf, C.byref(r), C.byref(mode)) == 0, L.lt_last_error()
        m, rr, taps = G.seg_taps(sigma)
        assert (mode.value, r.value) == (m, rr)
        assert torch.equal(torch.tensor(list(buf)[:taps.numel()], dtype=torch.float32).view(torch.int32), taps.view(torch.int32)), sigma
    assert L.lt_op_seg_taps(0.0, buf, C.byref(r), C.byref(mode)) != 0 and b"not positive" in L.lt_last_error()


@pytest.mark.parametrize("Hp,grid_w,blur_w,taps", [(2, 2, 2, (1, 2, 1)), (5, 9, 9, (1, 4, 6, 4, 1)), (4, 6, 5, (1, 4, 6, 4, 1)), (9, 5, 5, (1, 2, 1)),
                                                 (3, 4, 3, (1, 2, 1))])
def test_blur_restatement_equals_the_dense_matrix(Hp, grid_w, blur_w, taps):
    # dyadic taps and integer queries: every float64 sum is exact in any order, so the two forms agree bit for bit
    w = [v / float(sum(taps)) for v in taps]
    g = torch.Generator().manual_seed(Hp * 100 + grid_w)
    q = torch.randint(-8, 9, (2, 3, Hp * grid_w, 8), generator=g).double()
    got = XS.blur_ref(q, grid_w, blur_w, w)
    M = XS.blur_matrix(Hp, grid_w, blur_w, w)
    assert torch.equal(got, torch.einsum("nm,bhmc->bhnc", M, q))
    assert torch.allclose(M.sum(1), torch.ones(Hp * grid_w, dtype=torch.float64), atol=0, rtol=0)
    img = M.view(Hp, grid_w, Hp, grid_w)
    assert float(img[:, :blur_w, :, blur_w:].abs().sum()) == 0.0          # an end-of-line token is nobody's neighbour
    if blur_w < grid_w:
        assert torch.equal(got.view(2, 3, Hp, grid_w, 8)[:, :, :, blur_w:], q.view(2, 3, Hp, grid_w, 8)[:, :, :, blur_w:])
    # reflection without repeating the edge: the corner's horizontal neighbours at -1 and +1 are both column 1
    r = (len(taps) - 1) // 2
    assert float(M[0, 1]) == w[r] * (w[r + 1] + w[r - 1])
    mean = XS.mean_ref(q, grid_w, blur_w).view(2, 3, Hp, grid_w, 8)
    assert torch.equal(mean[:, :, 0, 0], q.view(2, 3, Hp, grid_w, 8)[:, :, :, :blur_w].sum((2, 3)) / (Hp * blur_w))


def test_seg_table_and_layer_checks():
    tgrid = ODE(4, "midpoint", 4).t
    assert torch.equal(G.seg_table(tgrid, "midpoint", 2.0, (0.2, 0.8)), G.slg_table(tgrid, "midpoint", 2.0, (0.2, 0.8)))
    with pytest.raises(ValueError, match="smoothed-energy table has an entry that is not finite"):
        G.seg_table(tgrid, "midpoint", math.inf)
    with pytest.raises(ValueError, match="smoothed-energy table is None"):
        G.check_seg(None, tgrid, "midpoint")
    with pytest.raises(ValueError, match="smoothed-energy table has 3 entries"):
        G.check_seg([1.0] * 3, tgrid, "midpoint")
    assert G.check_seg_layers([2, 0], [3], 4) == ([2, 0], [3])
    assert G.check_seg_layers([0, 1, 2, 3], (), 4)[0] == [0, 1, 2, 3]      # may hold every layer
    for kw, word in ((dict(seg_layers=[1, 1]), "blur index 1 is repeated"), (dict(seg_layers=[4]), "blur index 4 is outside 0..3"),
                     (dict(seg_layers=[1.5]), "blur layer 1.5 is not an integer"), (dict(seg_layers=[1], skip_layers=[1]), "in the skip set and in the blur set"),
                     (dict(seg_layers=[1], skip_layers=[0, 1, 2, 3]), "skip set leaves no layer")):
        with pytest.raises(ValueError, match=word):
            G.check_seg_layers(kw["seg_layers"], kw.get("skip_layers", ()), 4)


def test_refuse_with_seg_names_every_companion():
    t = torch.ones(4)
    G.refuse_with_seg(None, "dopri5", rescale=0.5, pag=t)                  # off: nothing is refused
    G.refuse_with_seg(t, "rk4")
    for kw, word in ((dict(pag=t), "a seg table.*together with perturbed-attention guidance"), (dict(slg=t), "a seg table.*together with an slg table"),
                     (dict(method="dopri5"), "smoothed-energy guidance is built for the fixed-grid methods"),
                     (dict(method="abm2"), "smoothed-energy guidance is built for the fixed-grid methods"),
                     (dict(rescale=0.5), "a seg table.*rescale / norm_limit"), (dict(norm_limit=2.0), "a seg table.*rescale / norm_limit"),
                     (dict(reuse=t), "a seg table.*guidance reuse"), (dict(teacache=0.1), "a seg table.*step caching"),
                     (dict(mask=t), "a seg table.*inpainting mask")):
        with pytest.raises(ValueError, match=word):
            G.refuse_with_seg(t, **kw)


class _Stub:
    """a model whose forward is cheap and depends on every argument: blocks scale the state, a skipped block is left out, a blurred one
    contributes a factor that depends on sigma"""
    n_layers, cfg_channels = 4, 3

    def __init__(self):
        self.calls = []

    def forward(self, x, t, y, skip_layers=(), blur_layers=(), blur_sigma=None):
        self.calls.append((tuple(skip_layers), tuple(blur_layers), blur_sigma, x.shape[0]))
        h = x.float()
        for l in range(self.n_layers):
            if l in skip_layers:
                continue
            f = 0.25 + (1.0 / (1.0 + blur_sigma) if l in blur_layers else 0.0)
            h = h * (1.0 + 0.125 * (l + 1)) + f * y.float().view(-1, 1, 1, 1) - 0.0625 * t.view(-1, 1, 1, 1)
        return h.to(x.dtype)

    def forward_with_cfg(self, x, t, y, cfg_scale):
        half = x.shape[0] // 2
        o = self.forward(torch.cat([x[:half]] * 2), t, y).to(torch.bfloat16)
        c, u = o[:half, :3], o[half:, :3]
        g = u + cfg_scale * (c - u)
        return torch.cat([torch.cat([g, o[:half, 3:]], 1), torch.cat([g, o[half:, 3:]], 1)]).to(x.dtype)


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_host_loop_on_a_stub_model(method, dtype):
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    tgrid = ODE(4, method, 4).t
    n = 3 * stages
    w = torch.tensor(([4.0, 1.0, 3.0, 1.0, 2.5, 1.0] * 2)[:n])
    s = torch.tensor(([2.0, 0.0, 0.0, 1.5, -1.0, 3.0] * 2)[:n])
    z = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(3)).to(dtype).repeat(2, 1, 1, 1)
    y = torch.tensor([1.0, -1.0])
    m = _Stub()
    # every s == 0: the schedule loop, bit for bit, and no third evaluation
    got = G.sample_cfg_seg(m, z, tgrid, w, torch.zeros(n), [1, 2], 2.0, [3], method, y=y)
    assert torch.equal(got, G.sample_cfg_schedule(m, z, tgrid, w, method, y=y))
    assert not [c for c in m.calls if c[0] or c[1]]
    # Q empty: skip-layer guidance, bit for bit
    got = G.sample_cfg_seg(m, z, tgrid, w, s, [], 2.0, [1, 2], method, y=y)
    assert torch.equal(got, G.sample_cfg_slg(m, z, tgrid, w, s, [1, 2], method, y=y))
    # Q given: the third evaluation takes both sets and sigma, on the cond rows alone, only on the stages the table names; sigma matters
    m.calls.clear()
    seg = G.sample_cfg_seg(m, z, tgrid, w, s, [2, 0], 2.0, [3], method, y=y)
    assert [c for c in m.calls if c[0] or c[1]] == [((3,), (2, 0), 2.0, 1)] * int((s != 0).sum())
    assert not torch.equal(seg, got)
    assert not torch.equal(seg, G.sample_cfg_seg(m, z, tgrid, w, s, [2, 0], math.inf, [3], method, y=y))
    for bad, word in ((dict(seg_layers=[1], skip_layers=[1]), "disjoint"), (dict(seg_layers=[], skip_layers=[]), "both layer sets are empty"),
                      (dict(seg_layers=[4]), "outside 0..3"), (dict(seg_layers=[1], rescale=0.5), "rescale"), (dict(seg_layers=[1], reuse=[0] * n), "reuse"),
                      (dict(seg_layers=[1], sigma=0.0), "not positive")):
        layers, skip, sigma = bad.pop("seg_layers"), bad.pop("skip_layers", ()), bad.pop("sigma", 2.0)
        with pytest.raises(ValueError, match=word):
            G.sample_cfg_seg(m, z, tgrid, w, s, layers, sigma, skip, method, y=y, **bad)
    with pytest.raises(ValueError, match="packed batch"):
        G.sample_cfg_seg(m, [z[0], z[1]], tgrid, w, s, [1], 2.0, (), method, y=y)
