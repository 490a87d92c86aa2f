"""Mirror of ``lumina_next_t2i_mini/transport.py`` - the flat ``ODE`` class the mini package (sample.py:146,
sample_img2img.py:146-216) uses instead of Sampler/ode, including the img2img ``strength`` cut of the time grid
(transport.py:79-80).  The model-callable protocol and the engine fast path are those of transport.integrators.ode:
a bound ``forward_with_cfg`` of one of our engine-backed models runs the whole trajectory in one ``lt_sample_ode`` call.
``sample(..., mask=, x1=, noise=)`` is the inpainting form (transport/masked.py; not in the reference): one ``lt_sample_ode_masked`` call
for an engine-backed callable, the host loop ``sample_masked`` otherwise.  ``sample(..., cfg_table=)`` is a guidance schedule
(transport/guidance.py; not in the reference either): one ``lt_sample_ode_cfg_schedule`` call, or the host loop ``sample_cfg_schedule``;
``cfg_rescale=`` / ``cfg_norm_limit=`` add the per-sample factor of ``guided_rule`` to the guided stages (``lt_sample_ode_cfg_rule`` /
``sample_cfg_rule``; without ``cfg_table`` the table holds ``cfg_scale`` at every stage).  ``sampler_type`` ab2 / ab3 / abm2 / abm3
(transport/multistep.py; not in the reference): one model evaluation per interval, one ``lt_sample_ode_multistep`` call or the host loop
``multistep_odeint``; with an inpainting mask they are refused by name.  ``cfg_reuse=`` (one 0 / 1 flag per evaluation, ``guidance.cfg_reuse_table``)
is guidance reuse: one ``lt_sample_ode_cfg_reuse`` call or the host loop ``sample_cfg_reuse``; refused together with a rescale / norm limit.
``cfg_apg=dict(eta=, momentum=, norm_threshold=)`` / ``cfg_zero_star=True`` (with ``cfg_zero_init=K``) are the projected forms of
``guidance.guided_project``: one ``lt_sample_ode_cfg_project`` call or the host loop ``sample_cfg_project``.
``windows=(offsets, (win_h, win_w))`` / ``window_weights=`` is tiled (MultiDiffusion) sampling (transport/tiled.py; not in the reference):
``x`` is ONE canvas latent, every stage evaluates its windows as one ``forward_with_cfg`` of 2 n rows and fuses their predictions - one
``lt_sample_ode_tiled`` call or the host loop ``sample_tiled``; refused by name together with any of the features above.
``compose=table`` (``guidance.compose_table``: fp32 ``[stages, K]``) is composed guidance (transport/guidance.py; not in the reference):
``x`` has ``B'`` rows and the conditioning ``(K + 1) B'`` - K weighted prompts, then the base prompt; every stage is one plain ``forward`` of those
rows composed by ``guided_compose`` - one ``lt_sample_ode_compose`` call or the host loop ``sample_cfg_compose``; refused by name together with any
of the features above.

Not mirrored: ``use_sd3=True`` (drives a diffusers SD3Transformer2DModel, not a Lumina model - out of scope)."""
from __future__ import annotations

import math

import torch as th

from .integrators import ADAPTIVE_METHODS, FIXED_GRID_METHODS, _engine_target, adaptive_odeint, fixed_grid_odeint
from .guidance import (cfg_table, refuse_rule_with_reuse, rule_is_off, sample_cfg_multistep, sample_cfg_reuse, sample_cfg_reuse_multistep,
                       sample_cfg_rule, sample_cfg_schedule)
from .multistep import MASKED_REFUSAL, MULTISTEP_METHODS, multistep_odeint
from .masked import expand_operands, sample_masked


class ODE:
    """reference lumina_next_t2i_mini/transport.py:57-111"""

    def __init__(self, num_steps, sampler_type="euler", time_shifting_factor=None, t0=0.0, t1=1.0, use_sd3=False,
                 strength=1.0):
        if use_sd3:
            raise NotImplementedError("use_sd3 drives a diffusers SD3 transformer, not a Lumina model (out of scope)")
        self.t = th.linspace(t0, t1, num_steps)
        if time_shifting_factor:
            s = time_shifting_factor
            self.t = self.t / (self.t + s - s * self.t)
        if strength != 1.0:  # img2img: start from the partially noised image at t[int(n (1 - strength))] (transport.py:79-80)
            self.t = self.t[int(num_steps * (1 - strength)):]
        self.use_sd3 = use_sd3
        self.sampler_type = sampler_type
        self.t_round_to_state_dtype = True  # torchdiffeq casts t to the state dtype (see integrators.ode)
        self.use_engine = True  # masked and multistep sampling: False keeps the host loop (sample_masked) for an engine-backed callable too

    def _sample_masked(self, x, model, mask, x1, noise, model_kwargs):
        """inpainting (transport/masked.py): the blend after every full step; one engine call when the callable is engine-backed"""
        if mask is None or x1 is None or noise is None:
            raise ValueError("masked sampling needs mask, x1 and noise together")
        if self.sampler_type in MULTISTEP_METHODS:
            raise NotImplementedError(MASKED_REFUSAL.format(self.sampler_type))
        if self.sampler_type not in FIXED_GRID_METHODS:
            raise NotImplementedError(f"masked sampling is built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not "
                                      f"'{self.sampler_type}'")
        if len(self.t) < 2:
            raise ValueError("masked sampling needs at least 2 grid points")
        mask, x1, noise = expand_operands(x, mask, x1, noise)
        target = _engine_target(model)
        if target is not None and x.is_cuda and self.use_engine and hasattr(target[0], "_engine_sample_ode_masked"):
            owner, use_cfg = target
            return owner._engine_sample_ode_masked(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, mask, x1, noise,
                                                   dict(model_kwargs))
        return sample_masked(model, x, self.t, mask, x1, noise, self.sampler_type, **model_kwargs)

    def _sample_cfg_schedule(self, x, model, table, model_kwargs, rescale=0.0, norm_limit=math.inf, reuse=None, slg=None, slg_layers=(), pag=None, pag_layers=()):
        """a guidance schedule (transport/guidance.py): a scale per stage; one engine call when the callable is an engine-backed forward_with_cfg"""
        if self.sampler_type not in FIXED_GRID_METHODS + MULTISTEP_METHODS:
            raise NotImplementedError(f"guidance schedules are built for the fixed-grid methods {', '.join(FIXED_GRID_METHODS)}, not "
                                      f"'{self.sampler_type}'")
        rule_off = rule_is_off(rescale, norm_limit)
        if table is None:  # a rule without a table: one scale for every stage
            table = cfg_table(self.t, self.sampler_type, model_kwargs.get("cfg_scale", 1.0))
        if reuse is not None:  # guidance reuse: refused together with a rule and on a packed list, by name
            if isinstance(x, (list, tuple)):
                raise ValueError("guidance reuse (cfg_reuse) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_rule_with_reuse(rescale, norm_limit)
        if slg is not None:  # skip-layer guidance: refused by name on a packed list, with a rule, a reuse table, another method
            from .guidance import refuse_with_slg, sample_cfg_slg
            if isinstance(x, (list, tuple)):
                raise ValueError("skip-layer guidance (slg_table) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_with_slg(slg, self.sampler_type, rescale, norm_limit, reuse)
        if pag is not None:  # perturbed-attention guidance: refused by name with what skip-layer guidance refuses, and with an slg table
            from .guidance import refuse_with_pag, sample_cfg_pag
            if isinstance(x, (list, tuple)):
                raise ValueError("perturbed-attention guidance (pag_table) takes a tensor state; a packed batch (a list of latents) is not served")
            refuse_with_pag(pag, self.sampler_type, rescale, norm_limit, reuse, slg)
        target = _engine_target(model)
        if target is not None and target[1] and x.is_cuda and self.use_engine and hasattr(target[0], "_engine_sample_ode_cfg_schedule"):
            if pag is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 pag=pag, pag_layers=pag_layers, slg_layers=slg_layers)
            if slg is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 slg=slg, slg_layers=slg_layers)
            if reuse is not None:
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                                 reuse=reuse)
            if rule_off:  # the call it was before the rule existed
                return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs))
            return target[0]._engine_sample_ode_cfg_schedule(x, self.t, self.sampler_type, self.t_round_to_state_dtype, table, dict(model_kwargs),
                                                             rescale=rescale, norm_limit=norm_limit)
        owner = getattr(model, "__self__", None)
        if owner is None or getattr(model, "__name__", "") != "forward_with_cfg" or not hasattr(owner, "forward"):
            raise TypeError("cfg_table needs the bound forward_with_cfg of a model that also has forward (the conditional-only stages call it)")
        if pag is not None:
            return sample_cfg_pag(owner, x, self.t, table, pag, pag_layers, slg_layers, self.sampler_type, t_round=self.t_round_to_state_dtype,
                                  **model_kwargs)
        if slg is not None:
            return sample_cfg_slg(owner, x, self.t, table, slg, slg_layers, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if reuse is not None and self.sampler_type in MULTISTEP_METHODS:
            return sample_cfg_reuse_multistep(owner, x, self.t, table, reuse, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if reuse is not None:
            return sample_cfg_reuse(owner, x, self.t, table, reuse, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        if self.sampler_type in MULTISTEP_METHODS:
            return sample_cfg_multistep(owner, x, self.t, table, self.sampler_type, rescale=rescale, norm_limit=norm_limit,
                                        t_round=self.t_round_to_state_dtype, **model_kwargs)
        if rule_off:
            return sample_cfg_schedule(owner, x, self.t, table, self.sampler_type, t_round=self.t_round_to_state_dtype, **model_kwargs)
        return sample_cfg_rule(owner, x, self.t, table, self.sampler_type, rescale=rescale, norm_limit=norm_limit,
                               t_round=self.t_round_to_state_dtype, **model_kwargs)

    def sample(self, x, model, mask=None, x1=None, noise=None, cfg_table=None, cfg_rescale=0.0, cfg_norm_limit=math.inf, cfg_reuse=None,
               slg_table=None, slg_layers=(), teacache=None, teacache_coefficients=None, pag_table=None, pag_layers=(), cfg_apg=None,
               cfg_zero_star=False, cfg_zero_init=0, windows=None, window_weights=None, compose=None, seg_table=None, seg_layers=(),
               seg_sigma=None, **model_kwargs):
        if isinstance(x, tuple):
            raise NotImplementedError("tuple states are not part of the sampling path")
        if seg_table is not None:  # smoothed-energy guidance (transport/guidance.py): its refusals come first, by name; None: the call it was
            from .guidance import sample_seg_front
            return sample_seg_front(x, model, self.t, self.sampler_type, cfg_table, model_kwargs, seg_table, seg_layers, seg_sigma, slg_layers,
                                    t_round=self.t_round_to_state_dtype, use_engine=self.use_engine,
                                    project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None, compose=compose,
                                    windows=windows, rescale=cfg_rescale, norm_limit=cfg_norm_limit, reuse=cfg_reuse, slg=slg_table,
                                    teacache=teacache, mask=next((m for m in (mask, x1, noise) if m is not None), None), pag=pag_table)
        if compose is not None:  # composed guidance (transport/guidance.py): its refusals come first, by name
            from .guidance import sample_compose_front
            return sample_compose_front(x, model, self.t, self.sampler_type, model_kwargs, compose, t_round=self.t_round_to_state_dtype,
                                        use_engine=self.use_engine, cfg_table=cfg_table,
                                        rule=None if rule_is_off(cfg_rescale, cfg_norm_limit) else True, cfg_reuse=cfg_reuse, slg=slg_table,
                                        pag=pag_table, project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None,
                                        teacache=teacache, mask=next((m for m in (mask, x1, noise) if m is not None), None), windows=windows)
        if windows is not None:  # tiled (MultiDiffusion) sampling (transport/tiled.py): its refusals come first, by name
            from .tiled import sample_tiled_front
            return sample_tiled_front(x, model, self.t, self.sampler_type, model_kwargs, windows, window_weights,
                                      t_round=self.t_round_to_state_dtype, use_engine=self.use_engine, cfg_table=cfg_table,
                                      rule=None if rule_is_off(cfg_rescale, cfg_norm_limit) else True, cfg_reuse=cfg_reuse, slg=slg_table,
                                      pag=pag_table, project=True if (cfg_apg is not None or cfg_zero_star or cfg_zero_init) else None,
                                      teacache=teacache, mask=next((m for m in (mask, x1, noise) if m is not None), None))
        if window_weights is not None:
            raise ValueError("window_weights belongs to tiled sampling: pass windows=(offsets, (win_h, win_w)) too")
        if cfg_apg is not None or cfg_zero_star or cfg_zero_init:  # projected guidance: its refusals come first, by name
            from .guidance import sample_project_front
            return sample_project_front(x, model, self.t, self.sampler_type, cfg_table, model_kwargs, apg=cfg_apg, zero_star=cfg_zero_star,
                                        zero_init=cfg_zero_init, t_round=self.t_round_to_state_dtype, use_engine=self.use_engine,
                                        rescale=cfg_rescale, norm_limit=cfg_norm_limit, reuse=cfg_reuse, slg=slg_table, pag=pag_table,
                                        teacache=teacache, mask=next((m for m in (mask, x1, noise) if m is not None), None))
        if pag_table is not None:  # perturbed-attention guidance: its refusals come first, by name
            from .guidance import refuse_with_pag
            refuse_with_pag(pag_table, self.sampler_type, cfg_rescale, cfg_norm_limit, cfg_reuse, slg_table, teacache,
                            next((m for m in (mask, x1, noise) if m is not None), None))
            return self._sample_cfg_schedule(x, model, cfg_table, model_kwargs, cfg_rescale, cfg_norm_limit, cfg_reuse, None, slg_layers,
                                             pag_table, pag_layers)
        if teacache is not None:  # step caching (transport/cache.py); None: the call made without it
            from .cache import IDENTITY, check_cache_args, refuse_with_teacache
            refuse_with_teacache(self.sampler_type, packed=isinstance(x, list), cfg_table=cfg_table, cfg_rescale=cfg_rescale,
                                 cfg_norm_limit=cfg_norm_limit, cfg_reuse=cfg_reuse, slg=slg_table,
                                 mask=next((m for m in (mask, x1, noise) if m is not None), None))
            coef = IDENTITY if teacache_coefficients is None else teacache_coefficients
            check_cache_args(teacache, coef)
            target = _engine_target(model)
            if target is None or not hasattr(target[0], "_engine_sample_ode_teacache"):
                raise TypeError("step caching (teacache) needs the bound forward / forward_with_cfg of an engine-backed model: the rule probes "
                                "the head of every evaluation, which only the engine offers")
            return target[0]._engine_sample_ode_teacache(x, self.t, self.sampler_type, target[1], self.t_round_to_state_dtype, dict(model_kwargs),
                                                         teacache, coef)
        if cfg_table is not None or cfg_reuse is not None or slg_table is not None or not rule_is_off(cfg_rescale, cfg_norm_limit):
            if mask is not None or x1 is not None or noise is not None:
                raise NotImplementedError("a guidance schedule (or skip-layer guidance) and an inpainting mask are not served together")
            return self._sample_cfg_schedule(x, model, cfg_table, model_kwargs, cfg_rescale, cfg_norm_limit, cfg_reuse, slg_table, slg_layers)
        if mask is not None or x1 is not None or noise is not None:
            return self._sample_masked(x, model, mask, x1, noise, model_kwargs)
        target = _engine_target(model)
        if (target is not None and x.is_cuda and self.use_engine and self.sampler_type in MULTISTEP_METHODS and len(self.t) >= 2
                and x.dtype in (th.float32, th.bfloat16) and hasattr(target[0], "_engine_sample_ode_multistep")):
            owner, use_cfg = target
            return owner._engine_sample_ode_multistep(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype, dict(model_kwargs))
        if target is not None and x.is_cuda and self.sampler_type in FIXED_GRID_METHODS and len(self.t) >= 2:
            owner, use_cfg = target
            return owner._engine_sample_ode(x, self.t, self.sampler_type, use_cfg, self.t_round_to_state_dtype,
                                            dict(model_kwargs))
        device = x.device

        def _fn(t, y):
            tvec = th.ones(y.size(0)).to(device) * t  # transport.py:87
            return model(y, tvec, **model_kwargs)

        if self.sampler_type in MULTISTEP_METHODS:
            return multistep_odeint(_fn, x, self.t.to(device), self.sampler_type, t_round=self.t_round_to_state_dtype)
        if self.sampler_type in ADAPTIVE_METHODS:
            return adaptive_odeint(_fn, x, self.t.to(device), method=self.sampler_type)
        return fixed_grid_odeint(_fn, x, self.t.to(device), method=self.sampler_type)
