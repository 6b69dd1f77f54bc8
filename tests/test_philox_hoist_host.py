"""The Philox section of csrc/mci_device.h compiled for the HOST (g++; the one GPU builtin in it, the three-input xor, replaced by a
macro): the form with a block-uniform high index word (PhiloxHead / philox_lane / philox4x32_10_uniform) must give the four words of
philox4x32_10 for every (index, block, stream, key), with 10 and with 7 rounds, and the section must reproduce the Random123
known-answer vectors of tests/golden/golden.json (the hoisted form on those whose block word is one it can take, 0 .. NCH-1).  Both
instantiations the kernels use: NCH = 8 blocks per sample (52-bit draws) and NCH = 4 (the 32-bit stream)."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "mcintegration.jl_amd", "csrc", "mci_device.h")
BEGIN, END = "// >>> philox section", "// <<< philox section"

WRAP = r"""
#define __device__
#define __forceinline__ inline
#define __builtin_amdgcn_bitop3_b32(a, b, c, table) ((a) ^ (b) ^ (c)) /* table 0x96 */
namespace mci {
typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
template <int I> struct IC { static constexpr int value = I; };
%s
}
using namespace mci;
extern "C" void generic(const u32 *ctr, const u32 *key, u32 *out) {
    const u32x4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
template <int Cc> static u32x4 block(const PhiloxLane &L, const PhiloxHead<%d> &H, const RoundKeys<false> &K, u32 c) {
    if constexpr (Cc < %d) return c == (u32)Cc ? philox4x32_10_uniform<false, %d, Cc>(L, H, K) : block<Cc + 1>(L, H, K, c);
    else return u32x4{0u, 0u, 0u, 0u};
}
extern "C" void hoisted(const u32 *ctr, const u32 *key, u32 *out) {
    const PhiloxHead<%d> H = make_philox_head<%d>(key[0], key[1], ctr[1], ctr[3]);   // once per workgroup
    const PhiloxLane L = philox_lane(ctr[0], H);                                      // once per sample
    const u32x4 r = block<0>(L, H, make_round_keys<false>(key[0], key[1]), ctr[2]);  // per block
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
"""


def philox_section():
    text = open(HEADER).read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "csrc/mci_device.h: the marker lines %r ... %r around the Philox section are gone" % (BEGIN, END)
    lo, hi = text.index(BEGIN), text.index(END)
    assert lo < hi and "philox4x32_10_uniform" in text[lo:hi]
    return text[lo:hi]


@pytest.fixture(scope="module", params=[(10, 8), (7, 8), (10, 4), (7, 4)], ids=lambda p: "rounds%d-nch%d" % p)
def host_philox(request, tmp_path_factory):
    rounds, NCH = request.param
    d = tmp_path_factory.mktemp("philox%d_%d" % request.param)
    src, so = os.path.join(d, "philox_host.cpp"), os.path.join(d, "philox_host.so")
    with open(src, "w") as fh:
        fh.write(WRAP % ((philox_section(),) + (NCH,) * 5))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-DMCI_PHILOX_ROUNDS=%d" % rounds, "-shared", "-fPIC", src, "-o", so],
                   check=True)
    return rounds, NCH, C.CDLL(so)


def call(fn, ctr, key):
    c, k, o = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    fn(c, k, o)
    return [int(v) for v in o]


def test_hoisted_rounds_equal_the_generic_rounds_and_the_known_answers(host_philox, golden, oracle):
    rounds, NCH, lib = host_philox
    vectors = golden["philox4x32_10" if rounds == 10 else "philox4x32_7"]
    assert vectors
    for v in vectors:
        assert call(lib.generic, v["ctr"], v["key"]) == v["out"]
        if v["ctr"][2] < NCH:
            assert call(lib.hoisted, v["ctr"], v["key"]) == v["out"]
    assert any(v["ctr"][2] < NCH for v in vectors)
    rng = random.Random(20240229)
    edge = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    for i in range(10000):
        word = (lambda: rng.choice(edge)) if i % 16 == 0 else (lambda: rng.getrandbits(32))
        ctr, key = [word(), word(), rng.randrange(NCH), word()], [word(), word()]
        want = call(lib.generic, ctr, key)
        assert call(lib.hoisted, ctr, key) == want, (ctr, key)
        if i % 100 == 0:   # ... and the generic rounds are the oracle's
            assert oracle.philox(ctr, key, rounds=rounds) == want
