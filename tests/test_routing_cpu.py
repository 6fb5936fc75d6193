"""The launch router (csrc/compress.h route_quantize / route_dequantize) on the
CPU: which kernel serves which part of which slice.

The sweep asserts COVERAGE, not the implementation: every bucket is quantized
by exactly one desc, every element decoded exactly once, the lean kernels are
only chosen when their documented preconditions hold.  The hand-written table
pins the routing of the shapes the GPU byte-parity suite uses."""

import itertools
import random

import pytest
import torch

from torch_cgx_amd import _C
from torch_cgx_amd.ops import golden

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BUCKETS = [7, 8, 64, 120, 256, 512, 1000, 1024, 2048, 2056, 8192]
FAST, GENERIC, TWO_PASS, SUB = (_C.KIND_FAST, _C.KIND_GENERIC,
                                _C.KIND_TWO_PASS, _C.KIND_SUB)
SKIP, TAIL = _C.FLAG_SKIP_INCOMPLETE, _C.FLAG_TAIL_ONLY


def _ns(bucket):
    return [0, 1, bucket - 1, bucket, bucket + 1, 3 * bucket + 5]


def _esize(dtype):
    return 4 if dtype == torch.float32 else 2


def _ceil(a, b):
    return (a + b - 1) // b


def test_kind_numbering():
    # the engine consumes one seed per group in (bits, kind) order: the
    # numbering decides the bytes of a stochastic run
    assert (FAST, GENERIC, TWO_PASS, SUB) == (0, 1, 2, 3)
    assert (SKIP, TAIL) == (1, 2)


# ---------------------------------------------------------------------------
# quantize
# ---------------------------------------------------------------------------
def _check_quantize(slices, groups):
    """slices: [(in, out, fb, n, bits, bucket, skip)] with unique `in`."""
    keys = [(g[0], g[1]) for g in groups]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    by_in = {s[0]: (i, s) for i, s in enumerate(slices)}
    covered = {s[0]: [] for s in slices}  # in -> [(first bucket, count)]
    tails = {s[0]: 0 for s in slices}
    for bits, kind, descs, cum, any_residual, max_gpl in groups:
        assert len(cum) == len(descs) + 1 and cum[0] == 0
        order = [by_in[d[0]][0] for d in descs]
        assert order == sorted(order)  # input order inside a group
        want_residual = False
        want_gpl = 1
        for i, (p_in, p_out, p_fb, n, bucket, flags) in enumerate(descs):
            _, (s_in, s_out, s_fb, s_n, s_bits, s_bucket, s_skip) = by_in[p_in]
            assert (p_out, p_fb, n, bucket, bits) == \
                (s_out, s_fb, s_n, s_bucket, s_bits)
            assert bool(flags & SKIP) == s_skip
            span = cum[i + 1] - cum[i]
            full = n // bucket
            if flags & TAIL:
                assert kind == GENERIC and not s_skip and span == 1
                covered[p_in].append((full, 1))
                tails[p_in] += 1
                continue
            covered[p_in].append((0, span))
            want_residual |= s_skip and n % bucket != 0
            if kind in (FAST, SUB):
                # preconditions documented in compress.h
                assert bucket % 8 == 0 and bucket <= 2048
                assert p_in % 16 == 0 and p_fb == 0 and n >= bucket
                ng = bucket // 8
                small_pow2 = ng < 64 and (ng & (ng - 1)) == 0
                assert small_pow2 == (kind == SUB)
                assert span == full  # cum counts FULL buckets
                want_gpl = max(want_gpl, _ceil(ng, 64))
            elif kind == GENERIC:
                assert bucket % 8 == 0  # the fused kernel packs whole groups
            else:
                assert kind == TWO_PASS and bucket % 8 != 0
        assert any_residual == want_residual
        if kind == FAST:
            assert max_gpl == want_gpl
    for s_in, s_out, s_fb, n, bits, bucket, skip in slices:
        nb = n // bucket if skip else _ceil(n, bucket)
        spans = sorted(covered[s_in])
        # every bucket in [0, nb) exactly once
        pos = 0
        for first, count in spans:
            assert first == pos
            pos += count
        assert pos == nb
        # a tail-only desc exists iff a lean kernel took the full buckets,
        # a partial bucket remains and it is not skipped
        took_full = any(
            kind in (FAST, SUB) and any(d[0] == s_in for d in descs)
            for _, kind, descs, _, _, _ in groups)
        assert tails[s_in] == int(took_full and n % bucket != 0 and not skip)


def _quant_slice(idx, n, bits, bucket, aligned, fb, skip, esize):
    base = 0x100000 * (idx + 1)
    p_in = base if aligned else base + esize
    return (p_in, base + 0x40000, base + 0x80000 if fb else 0, n, bits,
            bucket, skip)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_sweep(dtype):
    es = _esize(dtype)
    for bits, bucket in itertools.product(range(1, 9), BUCKETS):
        for n, aligned, fb, skip in itertools.product(
                _ns(bucket), (True, False), (False, True), (False, True)):
            if fb and bucket % 8 != 0:
                continue  # rejected before routing
            sl = [_quant_slice(0, n, bits, bucket, aligned, fb, skip, es)]
            groups = _C.route_quantize(sl)
            if n == 0:
                assert groups == []
                continue
            _check_quantize(sl, groups)


def test_quantize_random_batches():
    rng = random.Random(1234)
    for _ in range(300):
        sl = []
        for i in range(rng.randint(1, 12)):
            bucket = rng.choice(BUCKETS)
            fb = rng.random() < 0.25 and bucket % 8 == 0
            sl.append(_quant_slice(
                i, rng.choice(_ns(bucket) + [rng.randint(1, 5 * bucket)]),
                rng.choice([1, 2, 3, 4, 8]), bucket, rng.random() < 0.7, fb,
                rng.random() < 0.3, rng.choice([2, 4])))
        live = [s for s in sl if s[3] > 0]
        _check_quantize(live, _C.route_quantize(sl))


# (n, bucket) -> [(kind, cum, [flags])]; 16B-aligned base, no feedback, no
# skip_incomplete.  Shapes of tests/test_gpu_kernels.py::CASES.
QUANT_ROWS = {
    (512, 512): [(FAST, [0, 1], [0])],
    (1024, 512): [(FAST, [0, 2], [0])],
    (1000, 512): [(FAST, [0, 1], [0]), (GENERIC, [0, 1], [TAIL])],
    (64, 64): [(SUB, [0, 1], [0])],
    (4096, 1024): [(FAST, [0, 4], [0])],
    (1 << 20, 512): [(FAST, [0, 2048], [0])],
    (1025, 2048): [(GENERIC, [0, 1], [0])],
    (7, 512): [(GENERIC, [0, 1], [0])],
    (131, 64): [(GENERIC, [0, 1], [TAIL]), (SUB, [0, 2], [0])],
    (1000, 1000): [(FAST, [0, 1], [0])],  # 1000 = 125 * 8
    (5000, 120): [(FAST, [0, 41], [0]), (GENERIC, [0, 1], [TAIL])],
    (9, 7): [(TWO_PASS, [0, 2], [0])],
    (100000, 8192): [(GENERIC, [0, 13], [0])],
    (1003, 50): [(TWO_PASS, [0, 21], [0])],
}


def test_gpu_cases_are_the_pinned_rows():
    from test_gpu_kernels import CASES
    assert set(CASES) == set(QUANT_ROWS) == set(DEQUANT_ROWS)


@pytest.mark.parametrize("n,bucket", list(QUANT_ROWS))
def test_quantize_pinned_rows(n, bucket):
    groups = _C.route_quantize([(0x1000, 0x2000, 0, n, 4, bucket, False)])
    got = [(kind, cum, [d[5] for d in descs])
           for _, kind, descs, cum, _, _ in groups]
    assert got == QUANT_ROWS[(n, bucket)]
    assert all(g[0] == 4 and not g[4] for g in groups)
    gpl = {(4096, 1024): 2, (1000, 1000): 2}.get((n, bucket), 1)
    assert all(g[5] == gpl for g in groups if g[1] == FAST)


def test_quantize_pinned_variants():
    # feedback, an unaligned base and bucket > 2048 each force the generic
    # kernel for the whole slice; skip_incomplete drops the tail desc and
    # reports the raw residual from the lean group
    for sl in [(0x1000, 0x2000, 0x3000, 1000, 4, 512, False),
               (0x1004, 0x2000, 0, 1000, 4, 512, False),
               (0x1000, 0x2000, 0, 5000, 4, 2056, False)]:
        [(bits, kind, descs, cum, resid, _)] = _C.route_quantize([sl])
        assert (kind, cum, descs[0][5], resid) == \
            (GENERIC, [0, _ceil(sl[3], sl[5])], 0, False)
    [(bits, kind, descs, cum, resid, _)] = _C.route_quantize(
        [(0x1000, 0x2000, 0, 1000, 4, 512, True)])
    assert (kind, cum, descs[0][5], resid) == (FAST, [0, 1], SKIP, True)
    [(bits, kind, descs, cum, resid, _)] = _C.route_quantize(
        [(0x1004, 0x2000, 0, 1000, 4, 512, True)])
    assert (kind, cum, descs[0][5], resid) == (GENERIC, [0, 1], SKIP, True)
    # groups: ascending (bits, kind); one seed each, in this order
    groups = _C.route_quantize([
        (0x1000, 0x2000, 0, 1000, 8, 512, False),
        (0x3000, 0x4000, 0, 1001, 2, 1001, False),
        (0x5000, 0x6000, 0, 130, 2, 64, False),
        (0x7000, 0x8000, 0, 4096, 2, 2048, False),
    ])
    assert [(g[0], g[1]) for g in groups] == \
        [(2, FAST), (2, GENERIC), (2, TWO_PASS), (2, SUB), (8, FAST),
         (8, GENERIC)]
    assert groups[0][5] == 4  # bucket 2048: 4 groups per lane


def _routes(n, bucket, bits=4, in_ptr=0x1000, fb=0, skip=False):
    groups = _C.route_quantize([(in_ptr, 0x2000, fb, n, bits, bucket, skip)])
    return [(kind, cum, [d[5] for d in descs], gpl)
            for _, kind, descs, cum, _, gpl in groups]


def test_stochastic_suite_routes():
    """Every shape of tests/test_gpu_stochastic.py lands in the kernel it is
    listed under there (its tables are imported, not copied)."""
    import test_gpu_stochastic as st
    gpls = {512: 1, 1024: 2, 1536: 3, 2048: 4, 520: 2, 24: 1, 1000: 2}
    assert {b for _, b in st.FAST_SHAPES} == set(gpls)
    for n, bucket in st.FAST_SHAPES:
        assert n % bucket == 0 and n // bucket >= 2
        full = [0, n // bucket]
        assert _routes(n, bucket) == [(FAST, full, [0], gpls[bucket])]
        assert _routes(n + st.FAST_TAIL, bucket) == [
            (FAST, full, [0], gpls[bucket]), (GENERIC, [0, 1], [TAIL], 1)]
    assert [b // 8 for b in st.SUB_BUCKETS] == [1, 2, 4, 8, 16, 32]
    for n, bucket in st.sub_shapes():
        want = [(SUB, [0, 5], [0], 1)]
        if n % bucket:
            want.insert(0, (GENERIC, [0, 1], [TAIL], 1))
        assert _routes(n, bucket) == want
    n, bucket = st.SUB_BIG
    assert _routes(n, bucket) == [(SUB, [0, n // bucket], [0], 1)]
    assert n // bucket > 4096 * 4  # more buckets than waves in the largest grid
    for n, bucket in st.GENERIC_SHAPES:
        assert n < bucket or bucket > 2048
        assert _routes(n, bucket) == [
            (GENERIC, [0, _ceil(n, bucket)], [0], 1)]
    for n, bucket in st.UNALIGNED_SHAPES:
        for es in (2, 4):  # one element past a 16-byte boundary
            assert _routes(n, bucket, in_ptr=0x1000 + es) == [
                (GENERIC, [0, _ceil(n, bucket)], [0], 1)]
    for n, bucket in st.EF_SHAPES:
        assert _routes(n, bucket, fb=0x3000) == [
            (GENERIC, [0, _ceil(n, bucket)], [0], 1)]
    for n, bucket in st.TWO_PASS_SHAPES:
        assert _routes(n, bucket) == [
            (TWO_PASS, [0, _ceil(n, bucket)], [0], 1)]
    assert [_routes(n, b, skip=True) for n, b in st.SKIP_SHAPES] == [
        [(FAST, [0, 1], [SKIP], 1)], [(SUB, [0, 16], [SKIP], 1)],
        [(GENERIC, [0, 0], [SKIP], 1)]]
    # one shape per kernel for the wide packs, every width
    for bits in st.WIDE_BITS:
        assert [[r[0] for r in _routes(n, b, bits)]
                for n, b in st.WIDE_SHAPES] == [
            [FAST, GENERIC], [GENERIC, SUB], [GENERIC], [TWO_PASS]]
    # two slices of one shape share one launch group, per kind
    assert [[r[0] for r in _routes(n, b)] for n, b in st.TWIN_SHAPES] == [
        [FAST], [SUB], [GENERIC], [TWO_PASS]]
    # the four slices of one call: fast + tail, sub, two-pass
    assert [[r[0] for r in _routes(n, b)] for n, b in st.MULTI_SLICES] == [
        [FAST], [FAST, GENERIC], [SUB], [TWO_PASS]]


# ---------------------------------------------------------------------------
# dequantize
# ---------------------------------------------------------------------------
def _check_dequantize(slices, groups, dtype, src_stride, nsrc, add):
    """slices: [(in, out, n, bits, bucket, skip)] with unique `in`."""
    unit = 4 if dtype == torch.float32 else 8
    keys = [(g[0], g[1]) for g in groups]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    by_in = {s[0]: (i, s) for i, s in enumerate(slices)}
    covered = {s[0]: [] for s in slices}  # in -> [(first elem, count)]
    for bits, kind, descs, total_groups, any_residual in groups:
        assert kind in (FAST, GENERIC)
        order = [by_in[d[0]][0] for d in descs]
        assert order == sorted(order)
        want_residual = False
        work = 0
        for p_in, p_out, n, stride, bucket, d_nsrc, d_add, flags in descs:
            _, (s_in, s_out, s_n, s_bits, s_bucket, s_skip) = by_in[p_in]
            assert (p_out, n, bucket, bits) == (s_out, s_n, s_bucket, s_bits)
            assert (stride, d_nsrc, d_add) == (src_stride, nsrc, int(add))
            assert bool(flags & SKIP) == s_skip
            nq = n // bucket * bucket if s_skip else n
            if flags & TAIL:
                assert kind == GENERIC
                covered[p_in].append((nq - nq % unit, nq % unit))
                work += 1
                continue
            work += _ceil(nq, 8)
            want_residual |= s_skip and n % bucket != 0
            if kind == FAST:
                assert bucket % 8 == 0 and nq < 2 ** 31
                covered[p_in].append((0, nq - nq % unit))
            else:
                covered[p_in].append((0, nq))
        assert total_groups == work
        assert any_residual == want_residual
    for s_in, s_out, n, bits, bucket, skip in slices:
        nq = n // bucket * bucket if skip else n
        pos = 0
        for first, count in sorted(covered[s_in]):
            assert first == pos and (count > 0 or nq < unit)
            pos += count
        assert pos == nq  # every element in [0, nq) exactly once


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_sweep(dtype):
    for bits, bucket in itertools.product(range(1, 9), BUCKETS):
        for n, aligned, skip in itertools.product(
                _ns(bucket), (True, False), (False, True)):
            out = 0x200000 + (0 if aligned else _esize(dtype))
            sl = [(0x100000, out, n, bits, bucket, skip)]
            for stride, nsrc, add in [(0, 1, False), (1 << 16, 3, True)]:
                groups = _C.route_dequantize(sl, dtype, stride, nsrc, add)
                if n == 0:
                    assert groups == []
                    continue
                _check_dequantize(sl, groups, dtype, stride, nsrc, add)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_random_batches(dtype):
    rng = random.Random(4321)
    for _ in range(200):
        sl = []
        for i in range(rng.randint(1, 12)):
            bucket = rng.choice(BUCKETS)
            sl.append((0x100000 * (i + 1), 0x100000 * (i + 1) + 0x80000,
                       rng.choice(_ns(bucket) + [rng.randint(1, 5 * bucket)]),
                       rng.choice([1, 2, 3, 4, 8]), bucket,
                       rng.random() < 0.3))
        live = [s for s in sl if s[2] > 0]
        _check_dequantize(live, _C.route_dequantize(sl, dtype, 0, 1, False),
                          dtype, 0, 1, False)


# (n, bucket) -> ([(kind, total_groups, [flags])] fp32, same for 16-bit)
_F = lambda n: (FAST, _ceil(n, 8), [0])
_T = (GENERIC, 1, [TAIL])
DEQUANT_ROWS = {
    (512, 512): ([_F(512)], [_F(512)]),
    (1024, 512): ([_F(1024)], [_F(1024)]),
    (1000, 512): ([_F(1000)], [_F(1000)]),
    (64, 64): ([_F(64)], [_F(64)]),
    (4096, 1024): ([_F(4096)], [_F(4096)]),
    (1 << 20, 512): ([_F(1 << 20)], [_F(1 << 20)]),
    (1025, 2048): ([_F(1025), _T], [_F(1025), _T]),
    (7, 512): ([_F(7), _T], [_F(7), _T]),
    (131, 64): ([_F(131), _T], [_F(131), _T]),
    (1000, 1000): ([_F(1000)], [_F(1000)]),
    (5000, 120): ([_F(5000)], [_F(5000)]),
    (9, 7): ([(GENERIC, 2, [0])], [(GENERIC, 2, [0])]),
    (100000, 8192): ([_F(100000)], [_F(100000)]),
    (1003, 50): ([(GENERIC, 126, [0])], [(GENERIC, 126, [0])]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,bucket", list(DEQUANT_ROWS))
def test_dequantize_pinned_rows(dtype, n, bucket):
    groups = _C.route_dequantize([(0x1000, 0x2000, n, 4, bucket, False)],
                                 dtype)
    got = [(kind, total, [d[7] for d in descs])
           for _, kind, descs, total, _ in groups]
    assert got == DEQUANT_ROWS[(n, bucket)][0 if dtype == torch.float32 else 1]
    assert all(g[0] == 4 and not g[4] for g in groups)


def test_dequantize_pinned_variants():
    # n % 8 == 4: ragged for the 16-bit kernels only
    assert len(_C.route_dequantize([(0x1000, 0x2000, 516, 4, 512, False)],
                                   torch.float32)) == 1
    assert len(_C.route_dequantize([(0x1000, 0x2000, 516, 4, 512, False)],
                                   torch.float16)) == 2
    # the lean kernel indexes with u32: nq >= 2^31 goes to the generic one,
    # whatever the alignment (the dequant fast path needs none)
    big = 2 ** 31
    for n, kinds in [(big - 8, [FAST]), (big, [GENERIC]), (big + 5, [GENERIC])]:
        groups = _C.route_dequantize([(0x1004, 0x2004, n, 4, 512, False)],
                                     torch.float32)
        assert [g[1] for g in groups] == kinds
    # skip_incomplete: nq is a bucket multiple, never ragged; the residual is
    # reported by the group that decodes the slice
    [(bits, kind, descs, total, resid)] = _C.route_dequantize(
        [(0x1000, 0x2000, 1025, 4, 64, True)], torch.float32)
    assert (kind, total, descs[0][7], resid) == (FAST, 128, SKIP, True)


# ---------------------------------------------------------------------------
# wire-layout size: the native helper and the golden model cannot disagree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_buffer_size_matches_golden_over_sweep(dtype):
    for bits, bucket, skip in itertools.product(range(1, 9), BUCKETS,
                                                (False, True)):
        for n in _ns(bucket) + [2 ** 31 + 5]:
            assert _C.buffer_size(n, dtype, bits, bucket, skip) == \
                golden.buffer_size(n, dtype, bits, bucket, skip), \
                (n, bits, bucket, skip)
