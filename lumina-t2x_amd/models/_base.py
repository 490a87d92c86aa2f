"""Engine plumbing shared by the model classes of every family: the modules only HOLD parameters under the
reference's state_dict keys; a forward call hands them to the HIP engine (csrc/) through the C ABI.  There is no
PyTorch implementation of the forward pass and no CPU fallback."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib
from ..engine import DiTEngine, EngineLimits, _refuse_if_capturing, _refusing


# Any (re-)registration of a Parameter OR of a sub-module anywhere (setattr of an nn.Parameter, load_state_dict(assign=True),
# `m.layers[0] = prebuilt_block`, ...) bumps this epoch; the cached flat MODULE lists below are rebuilt when it moves.  In-place edits
# and .to() / .half() conversions keep the Parameter objects and show up as a changed (data_ptr, version) pair instead; parameters
# that disappear without a registration (`del m.a.bias`, `m.a.bias = None`) show up because the signature is read from the live
# `_parameters` dicts of the cached modules, not from a cached parameter list (the round-3 form cached the parameters and
# was driven by the parameter hook alone - a pre-built sub-module swapped in, or a parameter removed, kept the engine on OLD weights).
_PARAM_EPOCH = [0]


def _on_parameter_registration(module, name, param):
    _PARAM_EPOCH[0] += 1
    return None


def _on_module_registration(module, name, submodule):
    _PARAM_EPOCH[0] += 1
    return None


torch.nn.modules.module.register_module_parameter_registration_hook(_on_parameter_registration)
torch.nn.modules.module.register_module_module_registration_hook(_on_module_registration)


class WeightWatch:
    """'did any weight change since the engine last loaded them?' at ~50 us per call instead of ~0.3 ms: the module tree (567
    parameters under ~230 modules for the 2B model) is walked once and the flat module list kept; every per-step call of a
    host-driven sampler (dopri5, SDE: the default of Next-DiT-ImageNet/sample.py) goes through this check."""

    def _watch_reset(self) -> None:
        self._watch_modules = None
        self._watch_epoch = -1

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda() / .half(): may swap the Parameter objects without registering them
        out = super()._apply(fn, *args, **kwargs)
        _PARAM_EPOCH[0] += 1
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        _PARAM_EPOCH[0] += 1
        return out

    def _signature(self):
        # REMOVING a sub-module fires no registration hook (ModuleList.pop / __delitem__, `del m.sub`, edits of `_modules`): the number of
        # children over the cached tree is the structural term that catches it - a removal shrinks its parent's `_modules`
        stale = getattr(self, "_watch_modules", None) is None or self._watch_epoch != _PARAM_EPOCH[0]
        if not stale and sum(len(m._modules) for m in self._watch_tree) != self._watch_children:
            stale = True
        if stale:
            self._watch_tree = list(self.modules())
            self._watch_children = sum(len(m._modules) for m in self._watch_tree)
            self._watch_modules = [m for m in self._watch_tree if m._parameters]
            self._watch_epoch = _PARAM_EPOCH[0]
        # (inference tensors carry no version counter: in-place edits of such parameters are not seen - rebuild the model then)
        return tuple((p.data_ptr(), -1 if p.is_inference() else p._version)
                     for m in self._watch_modules for p in m._parameters.values() if p is not None)


class EngineSamplers:
    """transport fast paths (integrators.ode.sample / integrators.sde.sample): a whole trajectory in one C-ABI call.  Each model class maps
    the kwargs of ITS forward / forward_with_cfg onto the engine once, in ``_engine_sampler_args(x, use_cfg, kw) -> (engine, step kwargs)``
    (every reference sub-project has a different kwarg set); both samplers share that mapping."""

    def _engine_sampler_args(self, x, use_cfg, kw):
        raise NotImplementedError

    def _engine_sample_ode(self, x, tgrid, method, use_cfg, t_round, kw):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        return eng.sample_ode(x, tgrid, method, use_cfg=use_cfg, t_round_to_state_dtype=t_round, **args)

    def _engine_sample_ode_multistep(self, x, tgrid, method, use_cfg, t_round, kw):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode_multistep (ab2 / ab3 / abm2 / abm3)"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        return eng.sample_ode_multistep(x, tgrid, method, use_cfg=use_cfg, t_round_to_state_dtype=t_round, **args)

    def _engine_sample_ode_masked(self, x, tgrid, method, use_cfg, t_round, mask, x1, noise, kw):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode_masked (inpainting; mask / x1 / noise shaped and typed like x)"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        return eng.sample_ode_masked(x, tgrid, mask, x1, noise, method, use_cfg=use_cfg, t_round_to_state_dtype=t_round, **args)

    def _engine_sample_ode_cfg_schedule(self, x, tgrid, method, t_round, table, kw, return_trajectory=True, rescale=0.0, norm_limit=math.inf,
                                        reuse=None, slg=None, slg_layers=(), pag=None, pag_layers=(), apg=None, zero_star=False, zero_init=0,
                                        seg=None, seg_layers=(), seg_sigma=None):
        """kwargs of forward_with_cfg -> lt_sample_ode_cfg_schedule (guidance schedules; ``cfg_scale`` in kw is ignored), or - with a
        rescale blend or a norm limit - lt_sample_ode_cfg_rule, or - with a reuse table - lt_sample_ode_cfg_reuse, or -
        with a table of skip-layer scales - lt_sample_ode_cfg_slg, or - with a table of perturbed-attention scales -
        lt_sample_ode_cfg_pag (``slg_layers`` then join the same third prediction), or - with a table of smoothed-energy scales -
        lt_sample_ode_cfg_seg (likewise), or - with ``apg`` / ``zero_star`` - lt_sample_ode_cfg_project"""
        from ..transport.guidance import (check_project, refuse_rule_with_reuse, refuse_with_pag, refuse_with_project, refuse_with_seg,
                                          refuse_with_slg, rule_is_off)
        packed = not isinstance(x, torch.Tensor)
        form = _refusing(check_project, apg, zero_star, zero_init)[0]
        _refusing(refuse_with_project, form, method=method, rescale=rescale, norm_limit=norm_limit, reuse=reuse, slg=slg, pag=pag, packed=packed)
        if seg is not None and form is not None:
            raise _lib.LuminaLibError("smoothed-energy guidance (a seg table) together with projected guidance is not served")
        companions = (
            (seg, "smoothed-energy guidance",
             lambda: refuse_with_seg(seg, method=method, rescale=rescale, norm_limit=norm_limit, reuse=reuse, slg=slg, pag=pag)),
            (pag, "perturbed-attention guidance",
             lambda: refuse_with_pag(pag, method=method, rescale=rescale, norm_limit=norm_limit, reuse=reuse, slg=slg)),
            (slg, "skip-layer guidance",
             lambda: refuse_with_slg(slg, method=method, rescale=rescale, norm_limit=norm_limit, reuse=reuse)),
            (reuse, "guidance reuse",
             lambda: refuse_rule_with_reuse(rescale, norm_limit)),
        )
        for given, name, check in companions:
            if given is not None:  # a companion table: tensor states only, and not beside what its check names
                if packed:
                    raise _lib.LuminaLibError(f"{name}: a packed batch (a list of latents) is not served")
                _refusing(check)
        kw.setdefault("cfg_scale", 1.0)
        eng, args = self._engine_sampler_args(x, True, kw)
        args.pop("cfg_scale", None)
        if form is not None:
            return eng.sample_ode_cfg_project(x, tgrid, table, method, apg=apg, zero_star=zero_star, zero_init=zero_init,
                                              t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        if seg is not None:
            if seg_sigma is None:
                raise _lib.LuminaLibError("smoothed-energy guidance: a seg table needs seg_sigma (> 0; inf: the mean query)")
            return eng.sample_ode_cfg_seg(x, tgrid, table, seg, seg_layers, seg_sigma, method, skip_layers=slg_layers,
                                          t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        if pag is not None:
            return eng.sample_ode_cfg_pag(x, tgrid, table, pag, pag_layers, method, skip_layers=slg_layers, t_round_to_state_dtype=t_round,
                                          return_trajectory=return_trajectory, **args)
        if slg is not None:
            return eng.sample_ode_cfg_slg(x, tgrid, table, slg, slg_layers, method, t_round_to_state_dtype=t_round,
                                          return_trajectory=return_trajectory, **args)
        if reuse is not None and method in _lib.ODE_MULTISTEP_METHODS:
            return eng.sample_ode_multistep_cfg_reuse(x, tgrid, method, table, reuse, t_round_to_state_dtype=t_round,
                                                      return_trajectory=return_trajectory, **args)
        if reuse is not None:
            return eng.sample_ode_cfg_reuse(x, tgrid, table, reuse, method, t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        if method in _lib.ODE_MULTISTEP_METHODS:  # one evaluation per interval: the table has len(tgrid) - 1 entries
            return eng.sample_ode_multistep(x, tgrid, method, use_cfg=True, table=table, rescale=rescale, norm_limit=norm_limit,
                                            t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        if rule_is_off(rescale, norm_limit):  # the call it was before the rule existed
            return eng.sample_ode_cfg_schedule(x, tgrid, table, method, t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        return eng.sample_ode_cfg_rule(x, tgrid, table, method, rescale=rescale, norm_limit=norm_limit, t_round_to_state_dtype=t_round,
                                       return_trajectory=return_trajectory, **args)

    _cond_names = ("cap_feats", "cap_mask")  # the conditioning arguments of forward / forward_with_cfg, in call order

    @torch.no_grad()
    def sample_ode_cfg_schedule(self, z, tgrid, table, *cond, method: str = "midpoint", return_trajectory: bool = False, rescale: float = 0.0,
                                norm_limit: float = math.inf, reuse=None, slg=None, slg_layers=(), pag=None, pag_layers=(), apg=None,
                                zero_star: bool = False, zero_init: int = 0, seg=None, seg_layers=(), seg_sigma=None, **step_kw):
        """A guided fixed-grid trajectory with a scale per stage in ONE engine call (lt_sample_ode_cfg_schedule): stage k of interval
        i evaluates ``forward_with_cfg`` at ``table[i * stages + k]``, or - at scale 1 exactly - the plain forward of the cond rows alone, at
        half the rows.  ``cond``: the family's conditioning as ``forward_with_cfg`` takes it (``cap_feats, cap_mask`` or ``y``) for all
        ``z.size(0)`` rows; ``step_kw``: its other keyword arguments (``cfg_scale`` is ignored).  ``transport.guidance.cfg_table`` builds tables
        for guidance intervals and schedules.  ``method``: euler / midpoint / rk4, or a multistep method ab2 / ab3 / abm2 / abm3 (one evaluation
        per interval, so a table of ``len(tgrid) - 1`` entries; lt_sample_ode_multistep).  ``rescale`` (a blend in [0, 1]) / ``norm_limit`` (> 0; inf: off): the guided stages multiply
        their guided channels by the per-sample factor of ``transport.guidance.guided_rule`` (lt_sample_ode_cfg_rule); at the
        defaults the call is the schedule call.  ``reuse`` (one 0 / 1 flag per table entry; ``transport.guidance.cfg_reuse_table``): guided stages
        with flag 1 evaluate the cond rows alone and reuse the cond - uncond difference of the last stage with flag 0 (lt_sample_ode_cfg_reuse,
        DESIGN 7k; refused together with a rule); ``None``: the call made without it.  ``slg`` (one skip-layer scale per table entry;
        ``transport.guidance.slg_table``) with ``slg_layers``: stages with ``slg != 0`` also evaluate the cond rows with those blocks left out
        and add ``slg * (cond - skip)`` (lt_sample_ode_cfg_slg; euler / midpoint / rk4; refused together with a rule or ``reuse``).
        ``pag`` (one perturbed-attention scale per table entry; ``transport.guidance.pag_table``) with ``pag_layers``: the third prediction
        runs those blocks with the identity as their self-attention map - and ``slg_layers``, if given, left out - under the one table
        (lt_sample_ode_cfg_pag; an ``slg`` table beside a ``pag`` table is refused by name).
        ``seg`` (one smoothed-energy scale per table entry; ``transport.guidance.seg_table``) with ``seg_layers`` and ``seg_sigma``: the third
        prediction runs those blocks' self-attention on queries Gaussian-blurred over the token grid at that width (``inf``: the mean query) -
        and ``slg_layers``, if given, left out (lt_sample_ode_cfg_seg; refused by name with what ``pag`` is refused with, and with ``pag``).
        ``apg=dict(eta=, momentum=, norm_threshold=)`` or ``zero_star=True`` (with ``zero_init=K``): the guided stages form their output by
        ``transport.guidance.guided_project`` - APG's momentum / norm clip / damped parallel part, or CFG-Zero*'s rescaled unconditional row
        with ``K`` intervals of zero velocity that evaluate nothing (lt_sample_ode_cfg_project; euler / midpoint / rk4; exclusive,
        and refused by name together with any of the companions above).
        Returns the last state, or all ``len(tgrid)`` states."""
        if len(cond) > len(self._cond_names):
            raise TypeError(f"sample_ode_cfg_schedule takes the conditioning {self._cond_names}, got {len(cond)} positional arguments")
        kw = dict(zip(self._cond_names, cond), **step_kw)
        self._mirror_attention_flags(kw)
        return self._engine_sample_ode_cfg_schedule(z, tgrid, method, True, table, kw, return_trajectory=return_trajectory, rescale=rescale,
                                                    norm_limit=norm_limit, reuse=reuse, slg=slg, slg_layers=slg_layers, pag=pag,
                                                    pag_layers=pag_layers, apg=apg, zero_star=zero_star, zero_init=zero_init, seg=seg,
                                                    seg_layers=seg_layers, seg_sigma=seg_sigma)

    @torch.no_grad()
    def sample_ode_teacache(self, z, tgrid, *cond, method: str = "euler", threshold: float = 0.0, coefficients=(0.0, 0.0, 0.0, 1.0, 0.0),
                            return_trajectory: bool = False, host_loop: bool = False, t_round: bool = True, **step_kw):
        """A fixed-grid trajectory under step caching (the TeaCache rule) in ONE engine call (lt_sample_ode_cached): an evaluation
        whose timestep-modulated first-block input moved little since the stack last ran leaves the L blocks out and adds the residual they
        produced then.  ``cond``: the family's conditioning, then ``cfg_scale`` - given (also by keyword): every evaluation is
        ``forward_with_cfg``'s; left out: the plain ``forward``'s.  ``threshold`` (>= 0; 0: every evaluation runs the stack, the trajectory is
        ``sample_ode``'s) and ``coefficients`` (five, highest power first; the default is the identity): ``transport.cache`` has the definition.
        ``host_loop``: run that definition (one probe and one evaluation call per stage) instead of the one call.  Leaves
        ``self.last_cache_stats`` = dict(stats [ncalls, 3] float64: rel, acc after the add, ran; hits; nfe; rows).  Returns the last state, or
        all ``len(tgrid)`` states."""
        from ..transport import cache as TC
        kw = self._guided_kw("sample_ode_teacache", z, cond, step_kw, "by step caching")
        _refusing(TC.check_cache_method, method)
        _refusing(TC.check_cache_args, threshold, coefficients)
        use_cfg = "cfg_scale" in kw
        if use_cfg:
            self._mirror_attention_flags(kw)
        eng, args = self._engine_sampler_args(z, use_cfg, kw)
        if host_loop:
            rows = []
            out = TC.sample_teacache(TC.EngineEvaluator(eng, use_cfg, args), z, tgrid, method, threshold=threshold, coefficients=coefficients,
                                     t_round=t_round, stats=rows)
            stats = torch.tensor([[r, a, float(ran)] for r, a, ran in rows], dtype=torch.float64).reshape(len(rows), 3)
            hits = int(sum(1 for r in rows if not r[2]))
            self.last_cache_stats = dict(stats=stats, hits=hits, nfe=len(rows), rows=(len(rows) - hits) * z.shape[0])
            return out if return_trajectory else out[-1]
        out, stats = eng.sample_ode_cached(z, tgrid, method, use_cfg=use_cfg, threshold=threshold, coefficients=coefficients,
                                           t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)
        self.last_cache_stats = dict(stats=stats, hits=eng.last_cache_hits(), nfe=eng.last_nfe(), rows=eng.last_eval_rows())
        return out

    def _engine_sample_ode_teacache(self, x, tgrid, method, use_cfg, t_round, kw, threshold, coefficients):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode_cached; all states"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        out, stats = eng.sample_ode_cached(x, tgrid, method, use_cfg=use_cfg, threshold=threshold, coefficients=coefficients,
                                           t_round_to_state_dtype=t_round, **args)
        self.last_cache_stats = dict(stats=stats, hits=eng.last_cache_hits(), nfe=eng.last_nfe(), rows=eng.last_eval_rows())
        return out

    def _guided_kw(self, who, x, cond, step_kw, served=None):
        """the keyword arguments of ``forward_with_cfg`` from the call ``who(x, t, *cond, **step_kw)``: ``cond`` is the family's conditioning,
        then ``cfg_scale``.  ``served`` (``None``: not tested here): the closing words of the refusal of a packed batch."""
        if served is not None and not isinstance(x, torch.Tensor):
            raise _lib.LuminaLibError(f"{who}: a packed batch (a list of latents) is not served {served}")
        names = self._cond_names + ("cfg_scale",)
        if len(cond) > len(names):
            raise TypeError(f"{who} takes {names}, got {len(cond)} positional arguments")
        return dict(zip(names, cond), **step_kw)

    def _guided_engine(self, who, x, kw, needs_scale=True):
        """(engine, step kwargs) of one guided evaluation, the module left as ``forward_with_cfg`` leaves it"""
        if needs_scale and "cfg_scale" not in kw:
            raise TypeError(f"{who} needs cfg_scale")
        self._mirror_attention_flags(kw)
        return self._engine_sampler_args(x, True, kw)

    def _mirror_attention_flags(self, kw):
        if hasattr(self, "layers") and "proportional_attn" in kw and len(self.layers) and hasattr(self.layers[0], "attention"):
            for layer in self.layers:  # what forward_with_cfg leaves on the module (reference model.py:891-899)
                layer.attention.base_seqlen = kw.get("base_seqlen") if kw["proportional_attn"] else None
                layer.attention.proportional_attn = kw["proportional_attn"]

    def _leave_step_flags(self, kw):
        """the step flags of ``forward_with_cfg`` in ``kw`` -> what that call leaves on the module for the plain ``forward`` that follows:
        the attention flags on every layer (``_mirror_attention_flags``) and the RoPE factors of the families that keep them.  Pops them;
        returns ``scale_factor`` / ``scale_watershed`` of a family whose plain forward does not read them off the module (Next-DiT)."""
        self._mirror_attention_flags(kw)
        kw.pop("proportional_attn", None)
        kw.pop("base_seqlen", None)
        rs, ntk = kw.pop("rope_scaling_factor", None), kw.pop("ntk_factor", None)
        if hasattr(self, "_rope"):  # the class-conditional families: both or neither (forward_with_cfg asserts it)
            if rs is not None or ntk is not None:
                assert rs is not None and ntk is not None
                self._rope = (float(rs), float(ntk))
        elif hasattr(self, "rope_scaling_factor"):  # Flag-DiT: each persists once overridden
            self.rope_scaling_factor = rs if rs is not None else self.rope_scaling_factor
            self.ntk_factor = ntk if ntk is not None else self.ntk_factor
        elif rs is not None or ntk is not None:
            raise TypeError(f"{type(self).__name__} takes no rope_scaling_factor / ntk_factor")
        return {k: kw.pop(k) for k in ("scale_factor", "scale_watershed") if k in kw}

    @torch.no_grad()
    def sample_flowedit(self, x_src, tgrid, noise, *cond, src_cfg: float = 1.5, tgt_cfg: float = 5.5, z=None, return_trajectory: bool = False,
                        cfg_channels: int = 3, **step_kw):
        """Prompt-driven editing by FlowEdit's inversion-free rule in ONE engine call (lt_sample_flowedit, DESIGN 7l;
        ``transport.edit.sample_flowedit`` around this model's plain ``forward`` is the definition).  ``x_src [B', C, H, W]``: the source latent;
        ``z``: the edit state at ``tgrid[0]`` (default ``x_src``); ``noise [len(tgrid) - 1, B', C, H, W]``: one draw per interval;
        ``cond``: the family's conditioning (``cap_feats, cap_mask`` or ``y``) for 4 B' rows ``[src_*, tgt_*, neg_src_*, neg_tgt_*]``;
        ``src_cfg`` / ``tgt_cfg``: the guidance scale of each branch, a float or one per interval.  ``step_kw``: the step flags of
        ``forward_with_cfg`` (``proportional_attn``, ``base_seqlen``, ``scale_factor``, ``scale_watershed``, ``rope_scaling_factor``, ``ntk_factor``),
        left on the module as that call leaves them before the plain forward runs.  A state that is not on a ROCm device runs the host loop.
        Returns the last state, or all ``len(tgrid)`` states."""
        from ..transport import edit as E
        if len(cond) > len(self._cond_names):
            raise TypeError(f"sample_flowedit takes the conditioning {self._cond_names}, got {len(cond)} positional arguments")
        kw = dict(zip(self._cond_names, cond), **step_kw)
        cond_kw = {k: kw[k] for k in self._cond_names if k in kw}
        n = len(E._grid32(tgrid)) - 1
        scales = E.flowedit_scales(n, src_cfg, tgt_cfg)
        x_src, z, noise = E.check_edit_operands(x_src, z, noise, n)
        Bp = x_src.shape[0]
        E.check_cond_rows(cond_kw, Bp)
        override = self._leave_step_flags(kw)
        if not x_src.is_cuda:
            if override:
                raise TypeError(f"sample_flowedit: {sorted(override)} reach the engine alone; the plain forward of the host loop takes none")
            states = E.sample_flowedit(self.forward, x_src, tgrid, noise, scales, z=z, cfg_channels=cfg_channels, **cond_kw)
            return states if return_trajectory else states[-1]
        rows = torch.empty((E.ROWS * Bp,) + tuple(x_src.shape[1:]), dtype=x_src.dtype, device=x_src.device)  # the evaluation's shape
        eng, args = self._engine_sampler_args(rows, False, kw)
        args.pop("cfg_scale", None)
        att = self.layers[0].attention if hasattr(self, "layers") and len(self.layers) and hasattr(self.layers[0], "attention") else None
        if att is not None and hasattr(att, "proportional_attn") and "proportional_attn" not in args:  # what this family's plain forward passes on
            args.update(proportional_attn=bool(att.proportional_attn), base_seqlen=att.base_seqlen)
        args.update(override)
        return eng.sample_flowedit(x_src, tgrid, noise, scales, z=z, cfg_channels=cfg_channels, return_trajectory=return_trajectory, **args)

    @torch.no_grad()
    def forward_with_cfg_rule(self, x, t, *cond, rescale: float = 0.0, norm_limit: float = math.inf, **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` under a rescale blend and / or a norm limit in ONE engine call
        (lt_forward_cfg_rule): ``transport.guidance.guided_rule`` on the model's output of all rows.  ``cond``: the conditioning,
        then ``cfg_scale`` (or ``cfg_scale=`` by keyword).  At the defaults the call is ``forward_with_cfg``.  Tensor states only."""
        from ..transport.guidance import rule_is_off
        kw = self._guided_kw("forward_with_cfg_rule", x, cond, step_kw, "under a guidance rule")
        if rule_is_off(rescale, norm_limit):
            return self.forward_with_cfg(x, t, **kw)
        eng, args = self._guided_engine("forward_with_cfg_rule", x, kw, needs_scale=False)
        return eng.forward_cfg_rule(x, t, rescale=rescale, norm_limit=norm_limit, **args)

    @torch.no_grad()
    def forward_with_cfg_project(self, x, t, *cond, apg=None, zero_star: bool = False, keep_momentum: bool = False, **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` under a projected form in ONE engine call (lt_forward_cfg_project,
        DESIGN 7q): ``transport.guidance.guided_project`` on the model's output of all rows.  ``cond``: the conditioning, then ``cfg_scale`` (or
        ``cfg_scale=`` by keyword).  ``keep_momentum`` (APG): continue from the momentum the last projected evaluation left - refused by name
        when none of this shape is stored, or the conditioning was prepared anew since.  With neither form the call is ``forward_with_cfg``.
        Tensor states only."""
        from ..transport.guidance import check_project
        kw = self._guided_kw("forward_with_cfg_project", x, cond, step_kw, "by projected guidance")
        if _refusing(check_project, apg, zero_star, who="forward_with_cfg_project")[0] is None:
            if keep_momentum:
                raise _lib.LuminaLibError("forward_with_cfg_project: keep_momentum belongs to APG (apg=dict(...))")
            return self.forward_with_cfg(x, t, **kw)
        eng, args = self._guided_engine("forward_with_cfg_project", x, kw)
        return eng.forward_cfg_project(x, t, apg=apg, zero_star=zero_star, keep_momentum=keep_momentum, **args)

    @torch.no_grad()
    def forward_with_cfg_reuse(self, x, t, *cond, reuse: bool = False, **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` in ONE engine call that keeps (``reuse=False``: the result is
        ``forward_with_cfg``'s) or reuses (``reuse=True``: the cond rows alone are evaluated) the cond - uncond difference of the guided channels
        (lt_forward_cfg_reuse).  ``cond``: the conditioning for all ``x.size(0)`` rows, then ``cfg_scale`` (or ``cfg_scale=`` by
        keyword).  A reuse with no difference of this shape kept since the conditioning was last prepared is refused by name.  Tensor states only."""
        kw = self._guided_kw("forward_with_cfg_reuse", x, cond, step_kw, "by guidance reuse")
        eng, args = self._guided_engine("forward_with_cfg_reuse", x, kw)
        return eng.forward_cfg_reuse(x, t, reuse=reuse, **args)

    @torch.no_grad()
    def forward_with_cfg_slg(self, x, t, *cond, slg_scale: float = 0.0, slg_layers=(), **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` with skip-layer guidance in ONE engine call (lt_forward_cfg_slg,
        DESIGN 7m): the cond rows are also evaluated with the blocks ``slg_layers`` left out (``k``), and the guided channels become
        ``u + cfg_scale (c - u) + slg_scale (c - k)``.  ``cond``: the conditioning for all ``x.size(0)`` rows, then ``cfg_scale`` (or by
        keyword).  ``slg_scale == 0`` is ``forward_with_cfg``.  Tensor states only."""
        kw = self._guided_kw("forward_with_cfg_slg", x, cond, step_kw, "by skip-layer guidance")
        eng, args = self._guided_engine("forward_with_cfg_slg", x, kw)
        return eng.forward_cfg_slg(x, t, slg_scale=slg_scale, slg_layers=slg_layers, **args)

    @torch.no_grad()
    def forward_with_cfg_seg(self, x, t, *cond, seg_scale: float = 0.0, seg_layers=(), seg_sigma: float = math.inf, skip_layers=(), **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` with smoothed-energy guidance in ONE engine call
        (lt_forward_cfg_seg): the cond rows are also evaluated with the blocks ``seg_layers`` run on queries blurred at width
        ``seg_sigma`` (and ``skip_layers`` left out), prediction ``b``; the guided channels are ``u + cfg_scale (c - u) + seg_scale (c - b)``.
        ``seg_scale == 0`` is ``forward_with_cfg``.  Tensor states only."""
        kw = self._guided_kw("forward_with_cfg_seg", x, cond, step_kw, "by smoothed-energy guidance")
        eng, args = self._guided_engine("forward_with_cfg_seg", x, kw)
        return eng.forward_cfg_seg(x, t, seg_scale=seg_scale, seg_layers=seg_layers, seg_sigma=seg_sigma, skip_layers=skip_layers, **args)

    @torch.no_grad()
    def forward_with_cfg_pag(self, x, t, *cond, pag_scale: float = 0.0, pag_layers=(), skip_layers=(), **step_kw):
        """``forward_with_cfg(x, t, <conditioning>, cfg_scale, **step_kw)`` with perturbed-attention guidance in ONE engine call
        (lt_forward_cfg_pag): the cond rows are also evaluated with the blocks ``pag_layers`` perturbed - their self-attention map
        replaced by the identity - and the blocks ``skip_layers`` left out (``p``), and the guided channels become
        ``u + cfg_scale (c - u) + pag_scale (c - p)``.  ``pag_scale == 0`` is ``forward_with_cfg``.  Tensor states only."""
        kw = self._guided_kw("forward_with_cfg_pag", x, cond, step_kw, "by perturbed-attention guidance")
        eng, args = self._guided_engine("forward_with_cfg_pag", x, kw)
        return eng.forward_cfg_pag(x, t, pag_scale=pag_scale, pag_layers=pag_layers, skip_layers=skip_layers, **args)

    # ---- tiled (MultiDiffusion) sampling: one canvas, the model on overlapping windows of it ---------------------
    def _tiled_engine(self, what, y, windows, weights, kw):
        """the engine with the window table ``windows = (offsets, (win_h, win_w))`` set for the canvas ``y [1, C, Hc, Wc]`` and the conditioning
        in ``kw`` prepared for the 2 n rows - rows 0 .. n-1 the window prompts, rows n .. 2n-1 the negative prompts; a conditioning of two rows
        (one prompt, one negative prompt) is expanded to n of each.  Returns (engine, step kwargs, n)."""
        from ..transport import tiled as T
        if not isinstance(y, torch.Tensor):
            raise _lib.LuminaLibError(f"{what}: a packed batch (a list of latents) is not served by tiled sampling")
        if "cfg_scale" not in kw:
            raise TypeError(f"{what} needs cfg_scale")
        if y.dim() != 4 or y.shape[0] != 1:
            raise _lib.LuminaLibError(f"{what} takes ONE canvas latent [1, C, Hc, Wc], got {tuple(y.shape)}")
        try:
            offsets, win_hw = windows
            win_hw = (int(win_hw[0]), int(win_hw[1]))
            offs = T.check_windows(offsets, win_hw, tuple(y.shape[2:]), None)
        except (TypeError, ValueError) as exc:
            raise _lib.LuminaLibError(f"{what}: windows = (offsets, (win_h, win_w)): {exc}") from None
        n = len(offs)
        for name in self._cond_names:
            v = kw[name]
            if v.shape[0] == 2 and n > 1:
                kw[name] = v.repeat_interleave(n, dim=0)
            elif v.shape[0] != 2 * n:
                raise _lib.LuminaLibError(f"{what}: {n} windows need 2 n = {2 * n} rows of {name} (the window prompts, then the negative prompts) or "
                                          f"2 rows (one of each, for every window), got {v.shape[0]}")
        self._mirror_attention_flags(kw)
        rows = torch.empty((2 * n, y.shape[1]) + win_hw, dtype=y.dtype, device=y.device)  # the evaluation's shape
        eng, args = self._engine_sampler_args(rows, True, kw)
        src = (tuple(offs), win_hw, tuple(y.shape[2:]), None if weights is None else (weights.data_ptr(), weights._version))
        if getattr(eng, "_windows_src", (None,))[0] != src or getattr(eng, "_windows_key", None) is None:
            eng._windows_src = (None,)
            eng.set_windows(offs, win_hw, tuple(y.shape[2:]), weights)
            eng._windows_src = (src, weights)  # (the tensor is kept: its address cannot pass to other weights)
        return eng, args, n

    @torch.no_grad()
    def forward_with_cfg_tiled(self, y, t, windows, *cond, weights=None, **step_kw):
        """One evaluation of a canvas ``y [1, C, Hc, Wc]`` through overlapping windows in ONE engine call (lt_forward_tiled, DESIGN 7r;
        ``transport.tiled.tiled_velocity`` around ``forward_with_cfg`` is the definition): ``windows = (offsets, (win_h, win_w))``
        (``transport.tiled.window_grid``), ``weights`` fp32 ``[win_h, win_w]`` (``window_weights``; ``None``: ones).  ``cond``: the family's
        conditioning for the 2 n rows (or for 2: one prompt and one negative prompt for every window), then ``cfg_scale``; ``step_kw``: the
        other keyword arguments of ``forward_with_cfg``.  ``t``: one stage time, or 2 n."""
        kw = self._guided_kw("forward_with_cfg_tiled", y, cond, step_kw)
        eng, args, n = self._tiled_engine("forward_with_cfg_tiled", y, windows, weights, kw)
        tv = torch.as_tensor(t, dtype=torch.float32, device=y.device).reshape(-1)
        return eng.forward_tiled(y, tv.expand(2 * n) if tv.numel() == 1 else tv, **args)

    @torch.no_grad()
    def sample_ode_tiled(self, z, tgrid, windows, *cond, method: str = "midpoint", weights=None, return_trajectory: bool = False,
                         t_round: bool = True, **step_kw):
        """The fixed-grid trajectory of ONE canvas latent ``z [1, C, Hc, Wc]`` in ONE engine call (lt_sample_ode_tiled, DESIGN 7r;
        ``transport.tiled.sample_tiled`` around ``forward_with_cfg`` is the definition): every stage evaluates the windows as one
        ``forward_with_cfg`` of 2 n rows and fuses their predictions; euler / midpoint / rk4 step the canvas.  Arguments as
        ``forward_with_cfg_tiled``.  Returns the last canvas, or all ``len(tgrid)`` canvases."""
        from ..transport.tiled import refuse_with_tiled
        kw = self._guided_kw("sample_ode_tiled", z, cond, step_kw)
        try:
            refuse_with_tiled(method)
        except NotImplementedError as exc:
            raise _lib.LuminaLibError(f"sample_ode_tiled: {exc}") from None
        eng, args, _ = self._tiled_engine("sample_ode_tiled", z, windows, weights, kw)
        return eng.sample_ode_tiled(z, tgrid, method, t_round_to_state_dtype=t_round, return_trajectory=return_trajectory, **args)

    def _engine_sample_ode_tiled(self, x, tgrid, method, t_round, windows, weights, kw):
        """kwargs of forward_with_cfg -> lt_sample_ode_tiled; all states"""
        eng, args, _ = self._tiled_engine("tiled sampling", x, windows, weights, kw)
        return eng.sample_ode_tiled(x, tgrid, method, t_round_to_state_dtype=t_round, **args)

    # ---- composed guidance: K weighted prompts and one base prompt per image --------------------------------------
    def _compose_engine(self, what, x, K, kw):
        """the engine with the conditioning in ``kw`` prepared for the ``(K + 1) B'`` rows of a composed evaluation of ``x [B', C, H, W]`` - prompt
        1's rows, ..., prompt K's, the base prompt's - and the step kwargs of the plain forward that evaluation is: the step flags of
        ``forward_with_cfg`` in ``kw`` are left on the module as that call leaves them (``_leave_step_flags``), as FlowEdit does."""
        if not isinstance(x, torch.Tensor):
            raise _lib.LuminaLibError(f"{what}: a packed batch (a list of latents) is not served by composed guidance")
        if x.dim() != 4:
            raise _lib.LuminaLibError(f"{what} takes a state [B', C, H, W], got {tuple(x.shape)}")
        rows = (K + 1) * x.shape[0]
        for name in self._cond_names:
            if name not in kw:
                raise TypeError(f"{what} needs the conditioning {self._cond_names}")
            if kw[name].shape[0] != rows:
                raise _lib.LuminaLibError(f"{what}: {x.shape[0]} image(s) under K = {K} prompts need (K + 1) B' = {rows} rows of {name} (prompt 1's, "
                                          f"..., prompt K's, the base prompt's), got {kw[name].shape[0]}")
        kw.pop("cfg_scale", None)  # the weights are the scales
        override = self._leave_step_flags(kw)
        shape = torch.empty((rows,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)  # the evaluation's shape
        eng, args = self._engine_sampler_args(shape, False, kw)
        args.pop("cfg_scale", None)
        att = self.layers[0].attention if hasattr(self, "layers") and len(self.layers) and hasattr(self.layers[0], "attention") else None
        if att is not None and hasattr(att, "proportional_attn") and "proportional_attn" not in args:  # what this family's plain forward passes on
            args.update(proportional_attn=bool(att.proportional_attn), base_seqlen=att.base_seqlen)
        args.update(override)
        return eng, args

    @torch.no_grad()
    def forward_with_compose(self, x, t, *cond, weights, cfg_channels: int = 3, **step_kw):
        """One composed evaluation of ``x [B', C, H, W]`` in ONE engine call (lt_forward_compose; ``transport.guidance.guided_compose``
        on this model's plain ``forward`` of the replicated rows is the definition): ``g = u + sum_k w_k (c_k - u)`` on the guided channels.
        ``cond``: the family's conditioning (``cap_feats, cap_mask`` or ``y``) for ``(K + 1) B'`` rows - prompt 1's rows, ..., prompt K's, then
        the base (negative / empty) prompt's; ``weights``: the K weights (a negative one negates its prompt); ``step_kw``: the step flags of
        ``forward_with_cfg``.  ``t``: one stage time, or ``(K + 1) B'``.  A state that is not on a ROCm device runs the host definition."""
        from ..transport import guidance as G
        if len(cond) > len(self._cond_names):
            raise TypeError(f"forward_with_compose takes the conditioning {self._cond_names}, got {len(cond)} positional arguments")
        kw = dict(zip(self._cond_names, cond), **step_kw)
        w = _refusing(G.check_compose, weights, rows=1, who="forward_with_compose")
        K = w.shape[1]
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            return self._compose_host(x, kw, K, lambda fn, c: G.guided_compose(
                fn(x.repeat(K + 1, 1, 1, 1), torch.as_tensor(t, dtype=torch.float32).reshape(-1).expand((K + 1) * x.shape[0]), **c), w, cfg_channels))
        eng, args = self._compose_engine("forward_with_compose", x, K, kw)
        tv = torch.as_tensor(t, dtype=torch.float32, device=x.device).reshape(-1)
        return eng.forward_compose(x, tv.expand((K + 1) * x.shape[0]) if tv.numel() == 1 else tv, w, cfg_channels=cfg_channels, **args)

    @torch.no_grad()
    def sample_ode_compose(self, z, tgrid, table, *cond, method: str = "midpoint", return_trajectory: bool = False, t_round: bool = True,
                           cfg_channels: int = 3, **step_kw):
        """The composed fixed-grid trajectory of ``z [B', C, H, W]`` in ONE engine call (lt_sample_ode_compose, DESIGN 7s;
        ``transport.guidance.sample_cfg_compose`` around this model's plain ``forward`` is the definition): every stage evaluates the state
        under the K prompts and the base prompt as one plain forward of ``(K + 1) B'`` rows and composes the predictions with its row of
        ``table [(len(tgrid) - 1) * stages, K]`` (``transport.guidance.compose_table``); euler / midpoint / rk4 step the ``B'`` rows.
        Arguments as ``forward_with_compose``.  Returns the last state, or all ``len(tgrid)`` states."""
        from ..transport import guidance as G
        if len(cond) > len(self._cond_names):
            raise TypeError(f"sample_ode_compose takes the conditioning {self._cond_names}, got {len(cond)} positional arguments")
        kw = dict(zip(self._cond_names, cond), **step_kw)
        try:
            G.refuse_with_compose(method, packed=True if not isinstance(z, torch.Tensor) else None)
        except NotImplementedError as exc:
            raise _lib.LuminaLibError(f"sample_ode_compose: {exc}") from None
        w = _refusing(G.check_compose, table, who="sample_ode_compose")
        K = w.shape[1]
        if not z.is_cuda:
            out = self._compose_host(z, kw, K, lambda fn, c: G.sample_cfg_compose(fn, z, tgrid, w, K, method, cfg_channels=cfg_channels, **c))
            return out if return_trajectory else out[-1]
        eng, args = self._compose_engine("sample_ode_compose", z, K, kw)
        return eng.sample_ode_compose(z, tgrid, w, method, t_round_to_state_dtype=t_round, return_trajectory=return_trajectory,
                                      cfg_channels=cfg_channels, **args)

    def _compose_host(self, x, kw, K, run):
        """the host definition around this model's plain ``forward``: the conditioning alone reaches it (a plain forward takes no step flags)"""
        kw.pop("cfg_scale", None)
        cond_kw = {k: kw.pop(k) for k in self._cond_names if k in kw}
        if kw:
            raise TypeError(f"composed guidance: {sorted(kw)} reach the engine alone; the plain forward of the host loop takes none")
        return run(self.forward, cond_kw)

    def _engine_sample_ode_compose(self, x, tgrid, method, t_round, table, kw):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode_compose; all states"""
        from ..transport.guidance import check_compose
        w = _refusing(check_compose, table)
        eng, args = self._compose_engine("composed guidance", x, w.shape[1], kw)
        return eng.sample_ode_compose(x, tgrid, w, method, t_round_to_state_dtype=t_round, **args)

    def _engine_sample_ode_adaptive(self, x, tgrid, method, use_cfg, t_round, kw, *, rtol, atol, first_step=None, max_steps=2 ** 31 - 1):
        """kwargs of forward_with_cfg / forward -> lt_sample_ode_adaptive; returns (states [len(tgrid), *x.shape], stats dict)"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        return eng.sample_ode_adaptive(x, tgrid, method, rtol=rtol, atol=atol, first_step=first_step, max_steps=max_steps, use_cfg=use_cfg,
                                       t_round_to_state_dtype=t_round, **args)

    def _engine_sample_sde(self, x, noise, steps, last_coef, method, last_step, use_cfg, kw):
        """kwargs of forward_with_cfg / forward -> lt_sample_sde; returns (engine, loop states [n_steps - 1, *x.shape], last-step state or None)"""
        eng, args = self._engine_sampler_args(x, use_cfg, kw)
        traj, final = eng.sample_sde(x, noise, steps, last_coef, method, last_step, use_cfg=use_cfg, **args)
        return eng, traj, final


class EngineBackedModel(EngineSamplers, WeightWatch, nn.Module):
    """Mixin-style base: subclasses set ``_variant`` and implement ``_engine_kwargs()``."""

    _variant: int = _lib.LT_VARIANT_NEXT_T2I

    def _init_engine_state(self) -> None:
        self.engine_limits = EngineLimits()
        self._engine: Optional[DiTEngine] = None
        self._weights_sig = None
        self._watch_reset()

    def _engine_kwargs(self) -> dict:
        raise NotImplementedError

    def _tokens(self, H: int, W: int) -> int:
        return (H // self.patch_size) * (W // self.patch_size)

    def engine(self, x: torch.Tensor, text_len: int = 0) -> DiTEngine:
        """Create / resize the engine for this call's shapes and make sure it holds the current weights."""
        if not x.is_cuda:
            raise _lib.LuminaLibError(
                f"{type(self).__name__}.forward needs tensors on a ROCm device: the MI355X engine has no CPU fallback")
        B, _, H, W = x.shape
        lim = self.engine_limits
        need = EngineLimits(max(lim.max_batch, B), max(lim.max_tokens, self._tokens(H, W)), max(lim.max_text, text_len))
        if self._engine is None or need != self._engine.limits or self._engine.device != x.device:
            # (before the old engine is dropped: its buffers may be what a graph the caller recorded earlier reads)
            _refuse_if_capturing(f"{type(self).__name__}: a new engine for this call's shapes (lt_create)")
            self._engine = None
            self._engine = DiTEngine(variant=self._variant, limits=need, device=x.device, **self._engine_kwargs())
            self.engine_limits = need
            self._weights_sig = None
        sig = self._signature()
        if sig != self._weights_sig:
            self._engine.load_state_dict(self.state_dict())
            self._weights_sig = sig
        return self._engine

    def parameter_count(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def get_fsdp_wrap_module_list(self):
        return list(self.layers)

    def get_checkpointing_wrap_module_list(self):
        return list(self.layers)
