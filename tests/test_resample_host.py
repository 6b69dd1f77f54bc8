"""CPU tests of the carried chains' resampler: the oracle's mirrors (mcio_resample_chains, mcio_resample_weighted) against the
independent long-double reference of tests/resample_cases.py over the whole case table -- which also proves the table fit for the kernel's
test (tests/test_hip_resample.py): float64 stays within the cap on picks the tolerance clause lets through --, the rule for a total
weight of zero or NaN (new chain c continues stored chain c % n_old, as resample_block has it), and the refusals of the two test hooks
(csrc/mci_debug.h mci_debug_resample, mci_debug_sweep_resample_lds), which need no device."""
import numpy as np
import pytest

import mcintegration_jl_amd as mci
import resample_cases as R
from test_sweep_leaves_host import bubble, discrete, offline


def groups():
    out = {}
    for c in R.cases():
        parts = c["id"].split("-")
        out.setdefault("-".join(parts[:2]) if parts[0] in ("w", "m") else parts[0], []).append(c)
    return out


GROUPS = groups()


def test_the_table_covers_what_it_is_for():
    cs = R.cases()
    assert {c["n_old"] for c in cs} == set(R.N_OLD)
    for path in (lambda c: c["w_chain"] is not None, lambda c: c["w_chain"] is None and c["nd"] <= 16, lambda c: c["w_chain"] is None and c["nd"] > 16):
        mine = [c for c in cs if path(c)]
        assert {c["n_old"] for c in mine if c["expect"] == "ref"} == set(R.N_OLD)
        assert any(c["nblocks"] > 1 and c["n_new"] > c["n_old"] for c in mine) and any(c["nblocks"] > 1 and 1 < c["n_new"] < c["n_old"] for c in mine)
        assert {c["expect"] for c in mine} == {"ref", "fallback", "mirror"}
    assert {c["nd"] for c in cs if c["w_chain"] is None} == set(R.ND)
    for c in cs:
        if c["nblocks"] > 1 and c["expect"] == "ref" and "tie" not in c["id"]:         # the blocks differ: a stride mix-up shows
            a = c["w_chain"] if c["w_chain"] is not None else c["curr"]
            assert c["n_old"] < 7 or "ones" in c["id"] or not np.array_equal(a[0], a[1]), c["id"]


@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g not in ("f", "i")))
def test_the_mirrors_pick_what_the_long_double_reference_picks(oracle, group):
    total = 0
    for c in GROUPS[group]:
        excused = R.check_picks(c, R.mirror(oracle, c), "mirror")
        print("%-28s %8d picks, %d within 2 gamma of a tie" % (c["id"], c["nblocks"] * c["n_new"], excused))
        total += c["nblocks"] * c["n_new"]
    assert total > 0


def test_a_total_of_zero_or_nan_spreads_the_new_chains_over_the_stored_ones(oracle):
    """resample_block's `!(W[n_old-1] > 0.0)` branch in both mirrors: without it the bisection ends on n_old - 1 for every chain"""
    assert len(GROUPS["f"]) >= 16
    for c in GROUPS["f"]:
        np.testing.assert_array_equal(R.mirror(oracle, c), R.fallback_picks(c), err_msg=c["id"])
        np.testing.assert_array_equal(R.reference(c)[2], R.fallback_picks(c), err_msg=c["id"])
    np.testing.assert_array_equal(oracle.resample_weighted(np.zeros(10), 10), np.arange(10))
    np.testing.assert_array_equal(oracle.resample_chains(np.zeros(10, dtype=np.int32), [0.0, 1.0], [1.0, 1.0], 10), np.arange(10))
    np.testing.assert_array_equal(oracle.resample_weighted([1.0, np.nan, 1.0, 1.0], 4), np.arange(4))
    np.testing.assert_array_equal(oracle.resample_weighted([0.0, 0.0, 0.0], 8), np.arange(8) % 3)


def test_an_exact_tie_goes_to_the_first_running_weight_above_the_target(oracle):
    """the x cases are what they are meant to be -- the running weight just below the pick EQUALS the target, in long double too -- and
    the mirrors take the chain behind the tie (`>`, not `>=`), with no pick to spare under the cap"""
    assert len(GROUPS["x"]) == 7
    for c in GROUPS["x"]:
        W, t, ref, _ = R.reference(c)
        for b in range(c["nblocks"]):
            assert ref[b, 0] >= 1 and W[b, ref[b, 0] - 1] == t[b, 0] and W[b, ref[b, 0]] == 2.0 ** 53, c["id"]
        np.testing.assert_array_equal(R.mirror(oracle, c), ref, err_msg=c["id"])
        assert R.CAP * ref.size < 1


def test_a_total_of_infinity_ends_every_bisection_on_the_last_stored_chain(oracle):
    """(what the kernel is held to in tests/test_hip_resample.py; here: that the table's +inf cases are what they are meant to be)"""
    for c in GROUPS["i"]:
        np.testing.assert_array_equal(R.mirror(oracle, c), np.full((c["nblocks"], c["n_new"]), c["n_old"] - 1), err_msg=c["id"])


def test_the_hooks_refuse_bad_arguments_without_a_device():
    eng = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2())
    curr, one = np.zeros((2, 5), dtype=np.int32), np.ones(3)
    for bad, match in ((dict(curr_old=np.zeros((0, 5), dtype=np.int32)), "0 blocks"),
                       (dict(curr_old=np.zeros((2, 0), dtype=np.int32)), "0 stored"),
                       (dict(n_new=0), "0 new"), (dict(n_new=-3), "-3 new"),
                       (dict(rw_now=np.ones(0), rw_used=np.ones(0)), "0 integrands"),
                       (dict(rw_now=np.ones(65), rw_used=np.ones(65)), "65 integrands")):
        kw = dict(dict(curr_old=curr, rw_now=one, rw_used=one, n_new=4), **bad)
        with pytest.raises(mci.MCIError, match=match):
            eng.resample(**kw)
    with pytest.raises(ValueError):
        eng.resample(curr, one, one, 4, w_chain=np.ones((2, 4)))
    with pytest.raises(mci.MCIError, match="offline"):              # good arguments get as far as the device
        eng.resample(curr, one, one, 4)
    with pytest.raises(mci.MCIError, match="offline"):
        eng.resample(curr, one, one, 4, w_chain=np.ones((2, 5)))


def test_the_sweeps_lds_limit_is_the_map_offset_less_the_partial_sums():
    """mci_debug_sweep_resample_lds needs no device.  `discrete` has the smallest map of the sweep tests' problems: a Discrete(1, 3)
    leaf leaves 144 doubles behind the partial sums, fewer than the resampler has threads, so a block of lds_w + 1 stored chains is still
    one chain per thread there; sphere2_padding's 1000-increment grid leaves 4128 (tests/test_hip_sweep_carry.py places its chain counts
    on both sides of both)"""
    sphere2 = offline(mci.Configuration(var=mci.Continuous(0.0, 1.0), dof=[[2], [3]]), mci.catalog.sphere2())
    small, mid, big = discrete().sweep_resample_lds(), sphere2.sweep_resample_lds(), bubble().sweep_resample_lds()
    print("lds_w: discrete", small, "sphere2_padding", mid, "bubble", big)
    assert 1 <= small < 256 < mid < big
    assert small % 2 == 0 and mid % 2 == 0                          # (the map block starts on 16 bytes)