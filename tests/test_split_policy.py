"""The tile-splitting policy (csrc/vpt_split_policy.cpp) through vpt_split_plan (include/vpt_kat.h): host arithmetic, no GPU.

tests/golden/split_plans.npz holds, per case, the per-tile costs (uint32 ticks, seeded), the wave slots, the kernel, the forced
k and the expected k[] and wave count.  The expected values were NOT produced by the code under test: they come from the policy
as it stood inside vpt_capi.hip before it was moved (the planning part of decide_split, lpt_makespan, load_factor and the gain
tables, compiled verbatim from that commit in a scratch harness that is not part of the repository; the wave count by the rule
of its build_split_table).  The move must not change a single factor, so the comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

PLANS = np.load(os.path.join(GOLDEN, "split_plans.npz"))


def _plan(vpt, kernel, cost, slots, forced_k):
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    k = np.full(cost.size, -1, dtype=np.int32)
    waves = C.c_int(-1)
    rc = vpt.hip.vpt_split_plan(kernel, cost.ctypes.data, cost.size, slots, forced_k, k.ctypes.data, C.byref(waves))
    assert rc == 0, vpt.hip.vpt_last_error()
    return k, waves.value


@pytest.mark.parametrize("name", [str(n) for n in PLANS["names"]])
def test_plan_is_the_one_the_policy_gave_before_it_moved(vpt, name):
    cost, want = PLANS[name + "_cost"], PLANS[name + "_k"].astype(np.int32)
    kernel, slots, forced_k, want_waves = (int(v) for v in PLANS[name + "_meta"])
    k, waves = _plan(vpt, kernel, cost, slots, forced_k)
    print(name, "tiles", cost.size, "split", int(np.count_nonzero(k)), "waves", waves, "largest k", int(k.max()))
    assert np.array_equal(k, want)
    assert waves == want_waves == int(np.sum(1 << want.astype(np.int64)))
    # what each case is there for
    if name in ("k1_full_uniform", "k1_full_spread15", "k1_all_zero"):   # 3.5 tiles per wave slot / nothing measured: left alone
        assert not k.any() and waves == cost.size
    if name in ("k1_rank_of_8_spread15", "k2_small_spread8", "k2_full_spread8"):   # short of waves, or K2's two waves per slot: split
        assert k.any() and waves > cost.size
    if name == "k1_one_costly_tile":
        assert not k[:-1].any() and k[-1] == 6 and waves == 499 + 64
    if name == "k1_zero_then_spread":   # tiles that own no pixel cost nothing and stay whole
        assert not k[cost == 0].any() and k.any()
    if forced_k >= 0:
        assert np.all(k == min(forced_k, 6)) and waves == cost.size << min(forced_k, 6)


def test_bad_arguments_are_refused(vpt):
    waves = C.c_int(0)
    k = np.zeros(4, dtype=np.int32)
    cost = np.ones(4, dtype=np.uint32)
    assert vpt.hip.vpt_split_plan(2, cost.ctypes.data, 4, 3072, -1, k.ctypes.data, C.byref(waves)) != 0
    assert vpt.hip.vpt_split_plan(0, None, 4, 3072, -1, k.ctypes.data, C.byref(waves)) != 0
    assert vpt.hip.vpt_split_plan(0, cost.ctypes.data, 4, 0, -1, k.ctypes.data, C.byref(waves)) != 0
