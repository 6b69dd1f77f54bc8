"""The cursor section of csrc/mci_device.h compiled for the HOST (g++): the rule that turns a ticket -- the number a wave's atomic add on
its block's cursor word returns, less the launch's base -- into a range of 128-sample units.  Pulls are simulated the way the kernel
makes them (a wave holds one pull in flight: it reads a ticket, stops if it lies beyond the last range, else issues the next pull and
works on the range) with the waves taking turns in random order.  Whatever the order, every unit of the block must be handed out
exactly once, in ranges that follow the taper (single units last, nothing larger than the big size), and the word must end at
base + tickets + waves: the value the host (mci_iteration_run) starts the next launch from without reading the word."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "mcintegration.jl_amd", "csrc", "mci_device.h")
BEGIN, END = "// >>> cursor section", "// <<< cursor section"

WRAP = r"""
#define __device__
#define __host__
namespace mci {
typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
%s
}
using namespace mci;
extern "C" u64 tickets(u64 units, u32 waves, u32 log2_big, u32 ones) {
    CursorRule r; r.units = units; r.waves = waves; r.log2_big = log2_big; r.ones = ones;
    return cursor_tickets(r);
}
extern "C" void range(u64 units, u32 waves, u32 log2_big, u32 ones, u64 ntickets, u64 t, u64 *out) {
    CursorRule r; r.units = units; r.waves = waves; r.log2_big = log2_big; r.ones = ones;
    cursor_range(r, ntickets, t, out[0], out[1]);
}
"""


def cursor_section():
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_device.h: the marker lines %r ... %r around the cursor section are gone" % (BEGIN, END)
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi and "cursor_range" in text[lo:hi] and "cursor_tickets" in text[lo:hi]
    return text[lo:hi]


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("cursor")
    src, so = os.path.join(d, "cursor_host.cpp"), os.path.join(d, "cursor_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % cursor_section())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.tickets.restype = C.c_uint64
    lib.tickets.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.range.restype = None
    lib.range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    return lib


def hand_out(lib, rng, units, waves, k, ones, base):
    """one launch on one block: returns (the ranges in ticket order, the word's final value)"""
    n = lib.tickets(units, waves, k, ones)
    word = base
    out = (C.c_uint64 * 2)()
    ranges = {}
    inflight = {}
    for w in range(waves):             # every wave's first pull, in any order
        inflight[w] = None
    order = list(range(waves))
    rng.shuffle(order)
    for w in order:
        inflight[w] = word
        word += 1
    live = list(range(waves))
    while live:
        w = live[rng.randrange(len(live))]
        t = inflight[w] - base
        if t >= n:                     # beyond the last range: the wave is through, with no pull in flight
            live.remove(w)
            continue
        inflight[w] = word             # the next pull goes out before the range is worked on
        word += 1
        lib.range(units, waves, k, ones, n, t, out)
        assert t not in ranges
        ranges[t] = (int(out[0]), int(out[1]))
    return [ranges[t] for t in range(n)], word, n


CASES = [(u, w) for u in (1, 2, 3, 7, 8, 9, 31, 32, 33, 95, 96, 97, 255, 256, 257, 545, 1000, 1023, 1024, 1025, 2047, 3000, 4097)
         for w in (8, 24, 64, 256)]


@pytest.mark.parametrize("k,ones", [(4, 4), (1, 1), (2, 3), (6, 2), (10, 1)])
def test_every_unit_is_handed_out_once_and_the_word_ends_where_the_host_expects(rule, k, ones):
    rng = random.Random(20240229 + 16 * k + ones)
    cases = CASES + [(rng.randrange(1, 5000), rng.choice([8, 16, 24, 40, 128, 256])) for _ in range(40)]
    for units, waves in cases:
        base = rng.choice([0, 1, 12345, 2 ** 32 - 3, 2 ** 40 + 17])
        ranges, word, n = hand_out(rule, rng, units, waves, k, ones, base)
        assert word == base + n + waves, (units, waves)            # tickets + one failed pull per wave: the next launch's base
        # consecutive tickets are consecutive ranges that tile [0, units)
        assert ranges[0][0] == 0 and ranges[-1][1] == units, (units, waves)
        for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
            assert a0 < a1 == b0 < b1, (units, waves)
        sizes = [b - a for a, b in ranges]
        assert max(sizes) <= 2 ** k
        assert all(s == 1 for s in sizes[-min(n, ones * waves):])   # the last ranges are single units
        assert all(x >= y for x, y in zip(sizes[1:], sizes[2:]))     # ... and sizes only shrink (the first range takes the remainder)
        if units > waves * (ones + 2 ** k - 2):                      # long blocks: everything before the taper in big ranges
            nbig = units - waves * (ones + 2 ** k - 2)
            assert sizes.count(2 ** k) >= nbig // 2 ** k and n <= (nbig + 2 ** k - 1) // 2 ** k + waves * (ones + k - 1)


def test_the_base_carries_over_consecutive_launches(rule):
    """three launches of different lengths on the same word: each starts from where the one before it left the word"""
    rng = random.Random(7)
    word = 0
    for units in (700, 33, 2500):
        ranges, end, n = hand_out(rule, rng, units, 24, 4, 4, word)
        assert end == word + n + 24 and sum(b - a for a, b in ranges) == units
        word = end
