"""CPU tests of the carried VEGAS+ allocation (mci_set_stratification_carry): the cell rule k_strat_remap moves a d_h from one plan
to another with -- the section of csrc/mci_static_kernels.h between its marker lines, compiled for the HOST -- against the rule written
out in numpy; the `carry` field of mci.Stratify; the two entry points in the ctypes table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mcintegration_jl_amd as mci
from mcintegration_jl_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "mcintegration.jl_amd", "csrc", "mci_static_kernels.h")
BEGIN, END = "// >>> strat remap cell rule", "// <<< strat remap cell rule"

WRAP = r"""
#define __host__
#define __device__
%s
extern "C" int cell(int j, int n_old, int n_new) { return strat_remap_cell(j, n_old, n_new); }
extern "C" long long index_of(const int *j, const int *n_old, const int *n_new, int ndim) { return strat_remap_index(j, n_old, n_new, ndim); }
"""

# plan pairs (old, new) in three draws: refine, coarsen, non-nested, identity (tests/test_hip_strat_carry.py runs the same on the GPU)
PAIRS_3D = [((5, 1, 3), (7, 2, 4)), ((5, 1, 3), (2, 1, 2)), ((5, 1, 3), (3, 3, 3)), ((5, 1, 3), (5, 1, 3))]


def remap_numpy(d_old, n_old, n_new):
    """d on plan n_old -> plan n_new: new hypercube h' (draw 0 fastest) takes the value of the old hypercube holding its centre, per draw
    new cell j of n' -> old cell floor((2 j + 1) n / (2 n')), in integers"""
    n_old, n_new = [int(v) for v in n_old], [int(v) for v in n_new]
    rest = np.arange(int(np.prod(n_new)), dtype=np.int64)
    h, stride = np.zeros_like(rest), 1
    for n, m in zip(n_old, n_new):
        j, rest = rest % m, rest // m
        h += ((2 * j + 1) * n) // (2 * m) * stride
        stride *= n
    return np.asarray(d_old)[h]


@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_static_kernels.h: the marker lines around the remap cell rule are gone"
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi and "strat_remap_cell" in text[lo:hi]
    d = tmp_path_factory.mktemp("strat_remap")
    src, so = os.path.join(d, "remap_host.cpp"), os.path.join(d, "remap_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % text[lo:hi])
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.cell.restype, lib.cell.argtypes = C.c_int, [C.c_int] * 3
    lib.index_of.restype, lib.index_of.argtypes = C.c_longlong, [C.POINTER(C.c_int)] * 3 + [C.c_int]
    return lib


def test_cell_rule_all_pairs_one_draw(host_rule):
    for n in range(1, 10):
        for m in range(1, 10):
            got = [host_rule.cell(j, n, m) for j in range(m)]
            want = remap_numpy(np.arange(n), [n], [m])
            assert got == list(want), (n, m, got, list(want))
            assert min(got) >= 0 and max(got) <= n - 1 and got == sorted(got)
            if m % n == 0:   # nested refinement: every old cell has m / n children
                assert got == [j // (m // n) for j in range(m)]
    # n = 2 -> n' = 4 has no centre on an edge; n = 3 -> n' = 2, j = 0 has (centre 1/4 = 3/4 of an old cell, (1 * 3) / 4 = 0), and
    # n = 2 -> n' = 3, j = 1 sits exactly on the edge 1/2: (3 * 2) / 6 = 1, the upper cell
    assert [host_rule.cell(j, 2, 4) for j in range(4)] == [0, 0, 1, 1]
    assert host_rule.cell(0, 3, 2) == 0 and host_rule.cell(1, 3, 2) == 2
    assert host_rule.cell(1, 2, 3) == 1
    # 64-bit products: cells near 2^31
    big = 2 ** 31 - 1
    assert host_rule.cell(big - 1, big, big) == big - 1 and host_rule.cell(big - 1, 1, big) == 0 and host_rule.cell(0, big, 1) == big // 2


@pytest.mark.parametrize("old,new", PAIRS_3D + [((40, 40), (64, 50))])
def test_index_rule_several_draws(host_rule, old, new):
    D = len(old)
    arr = C.c_int * D
    want = remap_numpy(np.arange(int(np.prod(old))), old, new)
    got = []
    for h in range(int(np.prod(new))):
        j, rest = [], h
        for m in new:
            j.append(rest % m)
            rest //= m
        got.append(host_rule.index_of(arr(*j), arr(*old), arr(*new), D))
    assert got == list(want)
    if old == new:
        assert got == list(range(len(got)))


def test_refining_keeps_every_familys_share():
    """why k_strat_remap does not rescale: with every new hypercube holding its parent's value, a family's share of sum d is the parent's"""
    rng = np.random.default_rng(3)
    d = rng.random(15)
    r = remap_numpy(d, (5, 1, 3), (10, 2, 9))
    fam = remap_numpy(np.arange(15), (5, 1, 3), (10, 2, 9))
    share = np.bincount(fam, weights=r, minlength=15) / r.sum()
    np.testing.assert_allclose(share, d / d.sum(), rtol=1e-14)


def test_stratify_carry_field():
    assert mci.Stratify().carry is False
    s = mci.Stratify(beta=0.5, nstrat=[2, 3], max_nhcube=100, carry=True)
    assert s.carry is True
    assert repr(s) == "Stratify(beta=0.5, nstrat=[2, 3], max_nhcube=100, carry=True)"
    assert repr(mci.Stratify()) == "Stratify(beta=0.75, nstrat=None, max_nhcube=16777216, carry=False)"
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="carry"):
            mci.Stratify(carry=bad)


class _NoEngine:
    def __call__(self, *a, **k):
        raise AssertionError("an engine was created before the refusal")


@pytest.mark.parametrize("solver", ["mcmc", "vegasmc"])
def test_carry_is_refused_with_the_chain_solvers_before_any_engine(solver):
    with pytest.raises(ValueError, match="solver"):
        mci.integrate("w[0] = x[0] * x[1];", solver=solver, var=mci.Continuous(0.0, 1.0), dof=[[2]], neval=1e4, niter=2,
                      stratify=mci.Stratify(carry=True), engine_factory=_NoEngine())


def test_entry_points_are_bound():
    sigs = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    assert sigs["mci_set_stratification_carry"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert sigs["mci_get_strat_carry"] == (C.c_int, [C.c_void_p, _lib.c_int32_p, _lib.c_int32_p])
    L = mci.lib()
    assert hasattr(L, "mci_set_stratification_carry") and hasattr(L, "mci_get_strat_carry")
    assert L.mci_abi_version() == _lib.ABI_VERSION   # (two functions more, no structure changed)
    hooks = {name: args for name, _, args in _lib.DEBUG_SIGNATURES}
    for name in ("mci_debug_strat_alloc", "mci_debug_strat_reduce", "mci_debug_strat_remap"):     # (tests/test_strat_kernels_host.py holds their signatures)
        assert name in hooks and hasattr(L, name)
