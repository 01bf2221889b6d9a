"""ControlNet residuals of the FLUX forward, host side: the sample index rule of the engine (mc_mmdit_controlnet_index,
pure host arithmetic) against the reference's expression, and the schedule recorded in the golden."""
import json
import math
import os

import numpy as np
import pytest

from magcache_amd import mmdit as MM


def reference_index(i, n_blocks, n_samples, repeat):
    """the rule of the reference's FLUX forward, restated with floating-point ceil as it computes it (the engine uses integer
    arithmetic): blocks share a sample in runs of ceil(n_blocks / n_samples); under repeat the samples cycle"""
    run = int(math.ceil(n_blocks / n_samples))
    return i % n_samples if repeat else i // run


@pytest.mark.parametrize("repeat", [False, True])
def test_index_rule_matches_the_reference_expression(repeat):
    refused = []
    for n in range(1, 58):
        for m in range(1, 58):
            want = [reference_index(i, n, m, repeat) for i in range(n)]
            # the engine refuses more samples than blocks and any index past the list (the reference's IndexError)
            if m > n or max(want) >= m:
                refused.append((n, m))
                for i in range(n):
                    with pytest.raises(ValueError):
                        MM.controlnet_sample_index(i, n, m, repeat)
                continue
            assert [MM.controlnet_sample_index(i, n, m, repeat) for i in range(n)] == want, (n, m)
    # ceil keeps i // interval inside the list whenever m <= n: only the surplus-sample pairs are refused
    assert refused == [(n, m) for n in range(1, 58) for m in range(n + 1, 58)]


def test_index_rule_refuses_bad_arguments():
    for args in ((0, 0, 1), (-1, 3, 1), (3, 3, 1), (0, 3, 0), (0, 3, -1)):
        with pytest.raises(ValueError):
            MM.controlnet_sample_index(*args)
    # FLUX.1-dev with the usual 5 + 10 ControlNet: ceil(19 / 5) = 4, ceil(38 / 10) = 4
    assert [MM.controlnet_sample_index(i, 19, 5) for i in (0, 3, 4, 18)] == [0, 0, 1, 4]
    assert [MM.controlnet_sample_index(i, 38, 10) for i in (0, 4, 37)] == [0, 1, 9]
    assert [MM.controlnet_sample_index(i, 19, 2, True) for i in (0, 1, 2, 18)] == [0, 1, 0, 0]


def test_golden_schedule_equals_the_host_rule(golden_dir):
    g = np.load(os.path.join(golden_dir, "flux_controlnet_golden.npz"))
    meta = json.loads(str(g["meta"]))
    base = json.loads(str(np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))["meta"]))
    n_double, n_single = base["cfg"]["num_layers"], base["cfg"]["num_single_layers"]
    assert set(meta["cases"]) == {"each", "repeat"}
    for name, c in meta["cases"].items():
        nd, ns, rep = c["n_double_samples"], c["n_single_samples"], c["blocks_repeat"]
        assert c["double_index"] == [MM.controlnet_sample_index(i, n_double, nd, rep) for i in range(n_double)]
        assert c["single_index"] == [MM.controlnet_sample_index(i, n_single, ns) for i in range(n_single)]
        assert g[name + "_outs"].dtype == np.float16 and g[name + "_outs"].shape[0] == base["steps"]
        assert g[name + "_skipped"].tolist() == np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))["skipped"].tolist()
    rep = meta["cases"]["repeat"]
    assert rep["blocks_repeat"] and rep["n_single_samples"] == n_single - 1 and n_single % rep["n_single_samples"] != 0
    assert meta["cases"]["each"]["single_index"][-1] == n_single - 1      # a sample lands on the last block
    assert g["double_q"].shape[0] == n_double and g["single_q"].shape[0] == n_single
    # the case in which controlnet_blocks_repeat is not the plain rule: the reference read 0, 1, 2, 0 on four double blocks
    r4 = meta["repeat4"]
    n, k = r4["num_layers"], r4["n_double_samples"]
    assert r4["blocks_repeat"] and n % k != 0
    assert r4["double_index"] == [MM.controlnet_sample_index(i, n, k, True) for i in range(n)]
    assert r4["plain_index"] == [MM.controlnet_sample_index(i, n, k, False) for i in range(n)] != r4["double_index"]
    assert g["repeat4_out"].dtype == np.float16
