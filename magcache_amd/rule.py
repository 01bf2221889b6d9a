"""The MagCache rule of the Python shims, once: what model.py (Wan2.1, VACE), wan22.py and mmdit.py (FLUX, HunyuanVideo,
Qwen-Image) do with the attributes the reference scripts patch onto the model class.  Host scalars only, float64, in the
reference's order: ratio = ratio * table[cnt], err += |1 - ratio|, compare.  The families differ in the columns of VARIANTS
and nowhere else; csrc/rule.cpp states the same rule for C callers."""
from collections import namedtuple

import numpy as np


def _gate_wan22(cnt, n, R, split, mode):
    """the split-step retention gates, MagCache4Wan2.2/magcache_generate.py:294-303"""
    if split is not None:
        if mode == "i2v":
            return not (cnt < int(split + (n - split) * R))
        return not (cnt < int(split * R) or (cnt <= ((n - split) * R + split) and cnt >= split))
    return not (cnt < int(n * R))


# slots        1: scalar accumulators, one residual; 2: two-element lists, slot cnt % 2 (cond / uncond calls alternate)
# gate         (cnt, num_steps, retention_ratio, split_step, mode) -> the rule looks at this call
# strict       err < thresh, else err <= thresh
# veto         (cnt, num_steps) -> never skip this call; None: no such call
# wrap_resets  the accumulators start over when cnt wraps (Qwen-Image: the counter only)
# residual     the attribute that holds the cached residual(s)
# on_class     state is written to the model's class (Wan2.2: both experts share it), else to the instance
# fresh        the attribute groups (see fresh_state) the family's init sets for (cached, calibration) sampling
Variant = namedtuple("Variant", "slots gate strict veto wrap_resets residual on_class fresh")
_RUN, _CALIB, _ALL = ("cnt", "acc", "res"), ("cnt", "res", "stats"), ("cnt", "acc", "res", "stats")
VARIANTS = {
    "wan21": Variant(2, lambda cnt, n, R, split, mode: cnt >= int(n * R), True, None, True, "residual_cache", False,
                     (_RUN, _ALL)),
    "wan22": Variant(2, _gate_wan22, True, None, True, "residual_cache", True, (_RUN, _CALIB)),
    "qwen": Variant(2, lambda cnt, n, R, split, mode: cnt >= int(n * R), True, None, False, "residual_cache", False,
                    (_RUN, _CALIB)),
    "flux": Variant(1, lambda cnt, n, R, split, mode: cnt >= int(R * n + 0.5), False,
                    lambda cnt, n: np.round(cnt * ((28 - 1) / (n - 1))).astype(int) == 11, True, "previous_residual", False,
                    (_ALL, _ALL)),
    "hunyuan": Variant(1, lambda cnt, n, R, split, mode: cnt >= int(R * n), False, None, True, "residual_cache", False,
                       (_ALL, _ALL)),
}
_ACC = ("accumulated_ratio", "accumulated_steps", "accumulated_err")
_STATS = ("norm_ratio", "norm_std", "cos_dis")


def _idle(v):
    """the accumulators with nothing accumulated (new objects on every call)"""
    return dict(zip(_ACC, ([1.0, 1.0], [0, 0], [0.0, 0.0]) if v.slots == 2 else (1.0, 0, 0)))


def _home(model, v):
    return type(model) if v.on_class else model


def _put(model, v, name, slot, value):
    if v.slots == 2:
        getattr(model, name)[slot] = value      # in place, on whichever object holds the list
    else:
        setattr(model, name, value)


def fresh_state(variant, calibration=False):
    """{attribute: value} of a new sample, as the family's init_* sets it for cached (False) or calibration (True) sampling;
    None: every attribute of either, what a geometry change starts over"""
    v = VARIANTS[variant]
    groups = dict(cnt=dict(cnt=0), acc=_idle(v), res={v.residual: [None, None] if v.slots == 2 else None},
                  stats={k: [] for k in _STATS})
    if v.slots == 1:
        groups["acc"]["accumulated_ratio"] = 1      # the integer the reference's patch sites write
    names = _ALL if calibration is None else v.fresh[bool(calibration)]
    return {k: x for g in names for k, x in groups[g].items()}


def init_state(cls, variant, calibration=False):
    for k, x in fresh_state(variant, calibration).items():
        setattr(cls, k, x)


def decide(model, variant):
    """One call of the rule -> (state slot, skip this forward)."""
    v = VARIANTS[variant]
    cnt = int(model.cnt)
    p = cnt % 2 if v.slots == 2 else 0
    at = (lambda a: a[p]) if v.slots == 2 else (lambda a: a)
    skip = False
    if v.gate(cnt, model.num_steps, model.retention_ratio, getattr(model, "split_step", None), getattr(model, "mode", None)):
        ratio = at(model.accumulated_ratio) * model.mag_ratios[cnt]
        steps = at(model.accumulated_steps) + 1
        err = at(model.accumulated_err) + np.abs(1 - ratio)
        for name, x in zip(_ACC, (ratio, steps, err)):
            _put(model, v, name, p, x)
        if ((err < model.magcache_thresh if v.strict else err <= model.magcache_thresh) and steps <= model.K
                and not (v.veto and v.veto(cnt, model.num_steps))):
            skip = True
        else:
            for name, x in _idle(v).items():
                _put(model, v, name, p, at(x))
    if skip and at(getattr(model, v.residual)) is None:
        raise RuntimeError("MagCache asked to skip before any residual was cached (retention_ratio too small?)")
    return p, skip


def store_residual(model, variant, slot, residual):
    v = VARIANTS[variant]
    _put(_home(model, v), v, v.residual, slot, residual)


def advance(model, variant, reset=True):
    """One call is over: bump the counter; at the end of the schedule it wraps and, unless the family (or `reset`) says
    otherwise, the accumulators start over -- the cached residuals stay.  True when it wrapped."""
    v = VARIANTS[variant]
    home = _home(model, v)
    home.cnt = int(model.cnt) + 1
    if home.cnt < model.num_steps:
        return False
    home.cnt = 0
    if reset and v.wrap_resets:
        for k, x in _idle(v).items():
            setattr(home, k, x)
    return True


def calibrate(model, variant, slot, calib_stats, residual):
    """What every calibration forward does after its CALIB run: from the first call that has a previous residual of its
    slot on (cnt >= slots), append the engine's three statistics rounded to 5 decimals; then cache the new residual.
    `calib_stats` / `residual` are the engine's calls for this slot.  Returns the raw statistics, or None."""
    v = VARIANTS[variant]
    home, stats = _home(model, v), None
    if int(home.cnt) >= v.slots:
        stats = calib_stats()
        for name, x in zip(_STATS, stats):
            getattr(home, name).append(round(x, 5))
    store_residual(model, variant, slot, residual())
    return stats
