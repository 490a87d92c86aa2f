"""SDE sampling fixture: tests/golden/sde_imagenet_tiny.npz - TEST INFRASTRUCTURE ONLY.

    python scripts/make_sde_golden.py        (authoring container: needs the reference checkout)

Runs the UNMODIFIED Next-DiT-ImageNet `Sampler.sample_sde` (transport/transport.py:285-344 over integrators.py:5-76) on the unmodified
tiny `DiT_Llama` of tests/golden/imagenet_tiny.npz (same config, weights seed and inputs), imported through oracle/ref_harness.py and the
stubs as oracle/make_golden.py does.  Nothing under oracle/ is edited.

Cases (6 steps each, forward_with_cfg at scale 4): Euler / "sigma" / Mean and Heun / "SBDM" / Tweedie.  The SBDM case runs on the
"VP" path: on "Linear" (and "GVP") create_transport forces eps = 0 for velocity prediction whatever is passed, the SBDM diffusion then
divides by t = 0 and the reference's own fp32 run is NaN from the first step on (tests/test_host_logic.py keeps those as "same NaN").  Per case
  ref        fp32 model, fp32 state
  refbf16    the reference module in bf16 (model.to(bfloat16)), bf16 state        (plain)
  refbf16ac  the same under torch.autocast("cpu", bfloat16)
and `noise`: the th.randn draws of the loop in step order (recorded by wrapping torch.randn while the reference runs; the three runs of a
case see the same seed, hence the same draws).  The loop states are stored per step; the last-step state separately (`*_last`: the
reference returns it in fp32 for Mean / Tweedie whatever the state dtype).
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_fulldepth_golden as F  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CFG_SCALE = 4.0
NUM_STEPS = 6
CASES = {
    "euler_sigma_mean": dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04),
    "heun_sbdm_tweedie": dict(sampling_method="Heun", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Tweedie", last_step_size=0.04),
}
PATH = {"euler_sigma_mean": "Linear", "heun_sbdm_tweedie": "VP"}  # path_type of create_transport
SEED = 31


def bits(x):
    return x.to(torch.bfloat16).view(torch.int16).numpy().copy()


def run(sample_fn, z, model_fn, y):
    """one reference run under SEED with the loop's torch.randn draws recorded"""
    draws = []
    real = torch.randn

    def recording(*a, **k):
        out = real(*a, **k)
        draws.append(out.clone())
        return out

    torch.manual_seed(SEED)
    torch.randn = recording
    try:
        xs = sample_fn(z, model_fn, y=y, cfg_scale=CFG_SCALE)
    finally:
        torch.randn = real
    return xs, torch.stack(draws)


def main():
    torch.set_grad_enabled(False)
    assert R.available(), "needs the reference checkout (LUMINA_REFERENCE_ROOT)"
    os.environ["TORCHDYNAMO_DISABLE"] = "1"
    g = np.load(os.path.join(OUT, "imagenet_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    sd = synth.synth_state_dict(cfg, seed=int(g["seed_w"]))
    z, y = torch.from_numpy(g["z"]), torch.from_numpy(g["y"])
    z = z.to(torch.bfloat16).float()  # one input for every precision
    mod = F._fresh_import("Next-DiT-ImageNet", "models.models")
    model = mod.DiT_Llama(**cfg.ctor_kwargs()).eval()
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert np.allclose(model.forward_with_cfg(torch.from_numpy(g["z"]), torch.from_numpy(g["t"]), y, 4.0).numpy(), g["cfg4"], atol=1e-5)
    model_bf = mod.DiT_Llama(**cfg.ctor_kwargs()).eval()
    model_bf.load_state_dict(sd, strict=True)
    model_bf = model_bf.to(torch.bfloat16)
    tmod = F._fresh_import("Next-DiT-ImageNet", "transport")
    out = {"config": g["config"], "seed_w": g["seed_w"], "seed": SEED, "cfg_scale": CFG_SCALE, "num_steps": NUM_STEPS, "z": z.numpy(), "y": y.numpy(),
           "cases": np.array(json.dumps(CASES)), "paths": np.array(json.dumps(PATH))}
    for name, kw in CASES.items():
        tr = tmod.create_transport(PATH[name], "velocity", None, None, None)
        fn = tmod.Sampler(tr).sample_sde(num_steps=NUM_STEPS, **kw)
        xs, noise = run(fn, z, model.forward_with_cfg, y)
        assert len(xs) == NUM_STEPS and noise.shape[0] == NUM_STEPS - 1
        out[f"{name}_noise"] = noise.numpy()
        out[f"{name}_ref"] = torch.stack(xs[:-1]).numpy()
        out[f"{name}_ref_last"] = xs[-1].numpy()
        for ac, key in ((False, "refbf16"), (True, "refbf16ac")):
            with torch.autocast("cpu", torch.bfloat16, enabled=ac):
                xb, nb = run(fn, z.to(torch.bfloat16), model_bf.forward_with_cfg, y)
            assert torch.equal(nb, noise) and all(x.dtype == torch.bfloat16 for x in xb[:-1])
            out[f"{name}_{key}"] = bits(torch.stack(xb[:-1]))
            out[f"{name}_{key}_last"] = xb[-1].float().numpy()
            out[f"{name}_{key}_last_dtype"] = np.array(str(xb[-1].dtype))
            rel = [float((a.float() - b).norm() / b.norm()) for a, b in zip(xb, xs)]
            print(f"[{name}] {key} vs fp32 per step: " + " ".join(f"{r:.3e}" for r in rel) + f"  (last-step dtype {xb[-1].dtype})", flush=True)
    np.savez_compressed(os.path.join(OUT, "sde_imagenet_tiny.npz"), **out)
    print("sde_imagenet_tiny.npz written:", os.path.getsize(os.path.join(OUT, "sde_imagenet_tiny.npz")), "bytes")


if __name__ == "__main__":
    main()
