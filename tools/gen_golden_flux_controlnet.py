"""Generate tests/golden/flux_controlnet_golden.npz by RUNNING THE REFERENCE'S OWN magcache_forward /
magcache_calibration, with ControlNet samples, around the CPU FLUX restatement (oracle/flux_ref.py).

    python tools/gen_golden_flux_controlnet.py     (needs the reference checkout: MAGCACHE_REFERENCE, default /root/reference)

The two functions are read from MagCache4FLUX/magcache_flux.py at run time and exec'd with stub globals, exactly as
oracle/gen_golden_mmdit.py does for tests/golden/flux_forward_golden.npz; the model, its weights, the inputs and the
sigma schedule are that golden's, so the tests reuse its fixture.  Only controlnet_block_samples,
controlnet_single_block_samples and controlnet_blocks_repeat are new.

Cases (toy FLUX: 2 double + 3 single blocks, 108 image tokens, fp32; outputs stored as fp16):
  each     one sample per block (2 double, 3 single): the last single block adds one too
  repeat   controlnet_blocks_repeat=True with n - 1 samples (1 double, 2 single: 2 does not divide 3)
  calib    magcache_calibration statistics of `each`
  repeat4  the same toy with FOUR double blocks, one forward with controlnet_blocks_repeat=True and 3 double samples
           (the two of `each` and the first single one): the only case where repeat (samples 0, 1, 2, 0) and the plain
           rule (0, 0, 1, 1) read different samples
The samples are multiples of 1/64 (exact in bf16 and fp32, stored as int8 numerators).  The list index the reference
reads for every block is recorded by a list subclass and checked here against the engine's host rule.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from magcache_amd.mag_ratios import TABLES  # noqa: E402
from magcache_amd.mmdit import controlnet_sample_index  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402
from oracle.gen_golden_mmdit import fresh, reference_flux_functions  # noqa: E402


class Recording(list):
    """controlnet_*_samples as the reference indexes them, logging every index it reads"""

    def __init__(self, items, log):
        super().__init__(items)
        self.log = log

    def __getitem__(self, k):
        self.log.append(int(k))
        return super().__getitem__(k)


def main():
    torch.manual_seed(0)
    ref = reference_flux_functions()
    base = np.load(os.path.join(GOLD, "flux_forward_golden.npz"))
    meta = json.loads(str(base["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    steps, n_img = meta["steps"], meta["h2"] * meta["w2"]
    dim = cfg["attention_head_dim"] * cfg["num_attention_heads"]
    n_double, n_single = cfg["num_layers"], cfg["num_single_layers"]
    lat0, sig = torch.from_numpy(base["latent0"]), base["sigmas"]
    kw = dict(encoder_hidden_states=torch.from_numpy(base["ctx"]), pooled_projections=torch.from_numpy(base["pooled"]),
              img_ids=torch.from_numpy(base["img_ids"]), txt_ids=torch.from_numpy(base["txt_ids"]),
              guidance=torch.tensor([meta["guidance"]]), return_dict=False)
    g = torch.Generator().manual_seed(77)
    q_double = torch.randn(n_double, n_img, dim, generator=g).mul(4).round().clamp(-127, 127).to(torch.int8)
    q_single = torch.randn(n_single, n_img, dim, generator=g).mul(4).round().clamp(-127, 127).to(torch.int8)

    def patched(forward, cfg=cfg, seed=meta["weight_seed"]):
        cls = fresh(FR.FluxTransformer2DModel)
        model = FR.init_synthetic_(cls(**cfg), seed=seed, std=meta["weight_std"])
        cls.forward = forward
        cls.cnt, cls.num_steps = 0, steps
        cls.norm_ratio, cls.norm_std, cls.cos_dis = [], [], []
        cls.mag_ratios = ref.nearest_interp(np.asarray(TABLES["flux_dev"]), steps)
        cls.K, cls.magcache_thresh, cls.retention_ratio = meta["K"], meta["thresh"], meta["R"]
        cls.accumulated_ratio, cls.accumulated_err, cls.accumulated_steps = 1, 0, 0
        return cls, model

    def samples(nd, ns, log_d, log_s):
        return (Recording([q_double[i].float()[None] / 64 for i in range(nd)], log_d),
                Recording([q_single[i].float()[None] / 64 for i in range(ns)], log_s))

    def loop(forward, n_calls, nd, ns, repeat):
        cls, model = patched(forward)
        ran, skipped, outs, log_d, log_s = [], [], [], [], []
        hook = model.transformer_blocks[0].register_forward_hook(lambda *a: ran.append(1))
        cd, cs = samples(nd, ns, log_d, log_s)
        x = lat0.clone()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            for i in range(n_calls):
                n0 = len(ran)
                o = model(hidden_states=x, timestep=torch.tensor([float(sig[i])]), controlnet_block_samples=cd,
                          controlnet_single_block_samples=cs, controlnet_blocks_repeat=repeat, **kw)[0]
                skipped.append(len(ran) == n0)
                outs.append(o[0].numpy().copy())
                x = x + float(sig[i + 1] - sig[i]) * o
        hook.remove()
        # the index rule: what the reference read in every computed forward == the engine's host rule
        full = n_calls - sum(skipped)
        want_d = [controlnet_sample_index(i, n_double, nd, repeat) for i in range(n_double)]
        want_s = [controlnet_sample_index(i, n_single, ns) for i in range(n_single)]
        assert log_d == want_d * full and log_s == want_s * full, (log_d[:n_double], want_d, log_s[:n_single], want_s)
        return cls, skipped, np.stack(outs), want_d, want_s

    out, cases = {}, {}
    for name, nd, ns, repeat in (("each", n_double, n_single, False), ("repeat", n_double - 1, n_single - 1, True)):
        cls, skipped, outs, idx_d, idx_s = loop(ref.magcache_forward, steps, nd, ns, repeat)
        assert cls.cnt == 0 and sum(skipped) > 0
        assert skipped == [bool(s) for s in base["skipped"]], "ControlNet samples never enter the skip decision"
        out[name + "_outs"] = outs.astype(np.float16)
        out[name + "_skipped"] = np.array(skipped, dtype=np.int8)
        cases[name] = dict(n_double_samples=nd, n_single_samples=ns, blocks_repeat=repeat, double_index=idx_d, single_index=idx_s)
        print(name, "skipped", [int(s) for s in skipped], "moved the output by",
              float(np.linalg.norm(outs - base["outs"]) / np.linalg.norm(base["outs"])))
    cls, *_ = loop(ref.magcache_calibration, steps - 1, n_double, n_single, False)   # the lists clear when cnt wraps
    calib = dict(norm_ratio=list(cls.norm_ratio), norm_std=list(cls.norm_std), cos_dis=list(cls.cos_dis))

    # controlnet_blocks_repeat where it is not the plain rule: 4 double blocks, 3 samples
    cfg4, seed4 = dict(cfg, num_layers=4), 13
    three = [q[None].float() / 64 for q in (q_double[0], q_double[1], q_single[0])]
    outs4 = {}
    for repeat in (True, False):
        _, model = patched(ref.magcache_forward, cfg4, seed4)
        log_d = []
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            o = model(hidden_states=lat0.clone(), timestep=torch.tensor([0.5]),
                      controlnet_block_samples=Recording(three, log_d), controlnet_blocks_repeat=repeat, **kw)[0]
        assert log_d == [controlnet_sample_index(i, 4, 3, repeat) for i in range(4)] == ([0, 1, 2, 0] if repeat else [0, 0, 1, 1])
        outs4[repeat] = o[0].numpy().copy()
    moved = float(np.linalg.norm(outs4[True] - outs4[False]) / np.linalg.norm(outs4[False]))
    print("repeat4: repeat vs the plain rule moved the output by", moved)
    assert moved > 0.1
    out["repeat4_out"] = outs4[True].astype(np.float16)
    repeat4 = dict(num_layers=4, weight_seed=seed4, timestep=0.5, n_double_samples=3, blocks_repeat=True,
                   double_index=[0, 1, 2, 0], plain_index=[0, 0, 1, 1], moved_vs_plain_rule=round(moved, 4))
    path = os.path.join(GOLD, "flux_controlnet_golden.npz")
    np.savez_compressed(path, double_q=q_double.numpy(), single_q=q_single.numpy(),
                        meta=json.dumps(dict(sample_scale=1 / 64, cases=cases, calib=calib, repeat4=repeat4)), **out)
    print("  flux_controlnet_golden.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
