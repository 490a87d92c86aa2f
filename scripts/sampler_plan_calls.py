#!/usr/bin/env python3
"""One call of every guided sampler entry point and of every single-evaluation guidance / step-caching mode, on the tiny golden text model
(tests/golden/nextdit_tiny.npz): a 16 x 16 latent, batch 2, a 3-point grid, euler and midpoint (ab2 for the multistep entries).  Meant to be
run under a kernel trace (no counters) with one library and then another (LUMINA_DIT_LIB): the ordered kernel lists of the two runs are
compared, as profiles/sampler_plan/kernel_trace_diff.txt records.  Prints one JSON line: per call, the evaluations and rows the engine counted
and a checksum of the result, which two libraries that issue the same launches share.

    python scripts/sampler_plan_calls.py

Needs a GPU; not part of the test suite.  Reads nothing outside the repository."""
import hashlib
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lumina_t2x_amd  # noqa: E402,F401
from lumina_t2x_amd import models  # noqa: E402
from oracle import synth  # noqa: E402


def main():
    g = np.load(os.path.join(REPO, "tests", "golden", "nextdit_tiny.npz"), allow_pickle=False)
    cfg = synth.NextDiTConfig(**json.loads(str(g["config"])))
    model = models.NextDiT(**cfg.ctor_kwargs())
    model.load_state_dict(synth.synth_state_dict(cfg, seed=int(g["seed_w"])), strict=True)
    model = model.eval().to("cuda", torch.bfloat16)
    cap = torch.from_numpy(g["cap"])[:2].to("cuda", torch.bfloat16)
    mask = torch.from_numpy(g["mask"])[:2].cuda()
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(1, cfg.in_channels, 16, 16, generator=gen).repeat(2, 1, 1, 1).to("cuda", torch.bfloat16)
    t = torch.full((2,), 0.3, device="cuda")
    step = dict(proportional_attn=True, base_seqlen=16)
    tgrid = torch.tensor([0.0, 0.4, 1.0])
    out = {}

    def note(name, res):
        torch.cuda.synchronize()
        eng = model._engine
        res = res if isinstance(res, torch.Tensor) else torch.stack(list(res))
        digest = hashlib.sha256(res.float().cpu().numpy().tobytes()).hexdigest()[:16]
        out[name] = dict(nfe=eng.last_nfe(), rows=eng.last_eval_rows(), sha=digest)

    for method, stages in (("euler", 1), ("midpoint", 2)):
        n = 2 * stages
        table = torch.tensor([4.0, 1.0, 2.5, 1.0][:n] if stages == 2 else [4.0, 1.0])
        guided = torch.full((n,), 3.0)
        third = torch.tensor([2.0, 0.0, 1.5, 1.0][:n] if stages == 2 else [2.0, 0.0])
        flags = torch.tensor([0, 1, 1, 0][:n] if stages == 2 else [0, 1], dtype=torch.int32)

        def run(tab, **kw):
            return model.sample_ode_cfg_schedule(z, tgrid, tab, cap, mask, method=method, return_trajectory=True, **step, **kw)

        note(f"schedule {method}", run(table))
        note(f"rule {method}", run(table, rescale=0.5, norm_limit=10.0))
        note(f"reuse {method}", run(guided, reuse=flags))
        note(f"slg {method}", run(table, slg=third, slg_layers=(1,)))
        note(f"pag {method}", run(table, pag=third, pag_layers=(0,)))
        note(f"apg {method}", run(table, apg=dict(eta=0.0, momentum=-0.5, norm_threshold=15.0)))
        note(f"zero_star {method}", run(table, zero_star=True, zero_init=1))
        for host_loop in (False, True):  # lt_sample_ode_cached, then lt_forward_cached's probe / run / reuse under the host's controller
            note(f"teacache {method} host_loop={host_loop}",
                 model.sample_ode_teacache(z, tgrid, cap, mask, 4.0, method=method, threshold=1e9, return_trajectory=True, host_loop=host_loop, **step))
    two = torch.tensor([4.0, 1.0])
    note("multistep table", model.sample_ode_cfg_schedule(z, tgrid, two, cap, mask, method="ab2", return_trajectory=True, **step))
    note("multistep rule", model.sample_ode_cfg_schedule(z, tgrid, two, cap, mask, method="ab2", return_trajectory=True, rescale=0.5, **step))
    note("multistep reuse", model.sample_ode_cfg_schedule(z, tgrid, torch.full((2,), 3.0), cap, mask, method="ab2", return_trajectory=True,
                                                          reuse=torch.tensor([0, 1], dtype=torch.int32), **step))
    note("forward rule", model.forward_with_cfg_rule(z, t, cap, mask, 4.0, rescale=0.5, norm_limit=10.0, **step))
    apg = dict(eta=0.0, momentum=-0.5, norm_threshold=15.0)
    note("forward apg", model.forward_with_cfg_project(z, t, cap, mask, 4.0, apg=apg, **step))
    note("forward apg keep", model.forward_with_cfg_project(z, t, cap, mask, 4.0, apg=apg, keep_momentum=True, **step))
    note("forward zero_star", model.forward_with_cfg_project(z, t, cap, mask, 4.0, zero_star=True, **step))
    note("forward reuse store", model.forward_with_cfg_reuse(z, t, cap, mask, 4.0, reuse=False, **step))
    note("forward reuse again", model.forward_with_cfg_reuse(z, t, cap, mask, 4.0, reuse=True, **step))
    note("forward slg", model.forward_with_cfg_slg(z, t, cap, mask, 4.0, slg_scale=2.0, slg_layers=(1,), **step))
    note("forward slg cond", model.forward_with_cfg_slg(z, t, cap, mask, 1.0, slg_scale=2.0, slg_layers=(1,), **step))
    note("forward pag", model.forward_with_cfg_pag(z, t, cap, mask, 4.0, pag_scale=2.0, pag_layers=(0,), skip_layers=(1,), **step))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
