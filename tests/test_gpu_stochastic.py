"""Stochastic-rounding quantize on a real MI355X, byte for byte against the
golden model.

The kernels' random draw is a stateless hash of (seed, slice index in the
launch group, pack index in the slice); golden.stochastic_rand is its host
model, so a stochastic quantize has exactly one right answer and every
comparison here is torch.equal.  The shapes are the smallest that reach each
kernel path; tests/test_routing_cpu.py::test_stochastic_suite_routes holds
each one to the kernel it is listed under, so a shape that fell back to
another kernel fails there.

A single-slice _C.quantize call puts the slice at index 0 of every launch
group and hands every group the same seed.  The slice index and the per-group
seed are reached through _C.quantize_slices (several slices, one
route_quantize call, group k launched with seed + k, as
Engine::run_quantize does)."""

import numpy as np
import pytest
import torch

from torch_cgx_amd.ops import golden

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = [1, 2, 3, 4, 8]
WIDE_BITS = [5, 6, 7]  # packs wider than 32 bits: the 64-bit accumulator
SEEDS = [0, -1]        # -1: every high bit set once cast to uint64

# (n, bucket) per kernel path.  `n` of a k_quantize_fast / k_quantize_sub
# shape is a whole number of buckets; the tests add the ragged variant.
FAST_SHAPES = [
    (1536, 512),   # G=1, full wave
    (2048, 1024),  # G=2
    (3072, 1536),  # G=3: the MAXGT>2 kernel variant
    (4096, 2048),  # G=4
    (1040, 520),   # 65 packs: second stash row with one live lane
    (96, 24),      # 3 packs: idle lanes
    (3000, 1000),  # 1000 = 125 * 8, no two-pass bucket: G=2, 61 live lanes
]
FAST_TAIL = 5      # extra elements: the tail re-enters k_quantize (TAIL_ONLY)
SUB_BUCKETS = [8, 16, 32, 64, 128, 256]  # L = 1, 2, 4, 8, 16, 32
SUB_TAIL = 3
SUB_BIG = (1 << 20, 8)  # more buckets than waves in the grid; fp32 only
GENERIC_SHAPES = [
    (7, 512), (100, 512),  # n < bucket
    (4100, 4096),          # bucket > 2048: 8 packs per lane, 4 reloaded
    (8192 + 9, 8192),      # 16 packs per lane, 12 reloaded past the stash
]
UNALIGNED_SHAPES = [(520, 512), (1000, 64)]
EF_SHAPES = [(4096, 512), (1000, 64), (520, 512)]
TWO_PASS_SHAPES = [(9, 7), (1003, 50), (3000, 1001)]
SKIP_SHAPES = [(1000, 512), (1025, 64), (7, 512)]
# one shape per kernel for WIDE_BITS: (n, bucket)
WIDE_SHAPES = [(3072 + FAST_TAIL, 1536), (5 * 64 + SUB_TAIL, 64),
               (8192 + 9, 8192), (1003, 50)]

# the four slices of one quantize_slices call: (n, bucket)
MULTI_SLICES = [(1536, 512), (1029, 512), (320, 64), (1003, 50)]
# two identical slices in one launch group, per kernel kind: (n, bucket)
TWIN_SHAPES = [(1536, 512), (320, 64), (100, 512), (1003, 50)]


def sub_shapes():
    return [(5 * b + t, b) for b in SUB_BUCKETS for t in (0, SUB_TAIL)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _input(n, dtype, salt=0):
    """A seed per case: the size and the caller's salt (bits, slice number)."""
    torch.manual_seed(1009 * n + salt)
    return torch.randn(n).to(dtype)


def _assert_same_bytes(got, want, what):
    assert got.numel() == want.numel(), what
    if not torch.equal(got, want):
        diff = (got != want).nonzero().flatten()
        raise AssertionError(
            f"{len(diff)} of {got.numel()} bytes differ, first at "
            f"{diff[:10].tolist()}: {what}")


def _check(x, bits, bucket, skip=False):
    """Both seeds: the kernel's bytes are the model's."""
    from torch_cgx_amd import _C
    n = x.numel()
    xg = x.to(_dev())
    assert xg.data_ptr() % 16 == 0
    for seed in SEEDS:
        want = golden.quantize(x, bits, bucket,
                               rand=golden.stochastic_rand(seed, n),
                               skip_incomplete=skip)
        got = _C.quantize(xg, bits, bucket, True, seed, skip).cpu()
        _assert_same_bytes(got, want, (n, bucket, bits, x.dtype, seed, skip))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", FAST_SHAPES)
def test_fast_kernel(dtype, bits, n, bucket):
    """k_quantize_fast at every groups-per-lane count, and the same shape
    with a ragged tail, which k_quantize encodes under the slice-global pack
    index (kFlagTailOnly)."""
    _check(_input(n, dtype, bits), bits, bucket)
    _check(_input(n + FAST_TAIL, dtype, bits), bits, bucket)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", sub_shapes())
def test_sub_kernel(dtype, bits, n, bucket):
    """k_quantize_sub at every L; five buckets, so segments go inactive for
    L < 64, without and with a ragged tail."""
    _check(_input(n, dtype, bits), bits, bucket)


@pytest.mark.parametrize("bits", BITS)
def test_sub_kernel_more_buckets_than_waves(bits):
    """131072 buckets of 8 on a grid of 16384 waves: every wave takes eight
    buckets a grid stride apart."""
    n, bucket = SUB_BIG
    _check(_input(n, torch.float32, bits), bits, bucket)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", GENERIC_SHAPES)
def test_generic_kernel(dtype, bits, n, bucket):
    """k_quantize for n < bucket and for buckets past the register stash,
    whose packs are loaded again for the encode."""
    _check(_input(n, dtype, bits), bits, bucket)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", UNALIGNED_SHAPES)
def test_generic_kernel_unaligned_base(dtype, bits, n, bucket):
    """Input one element past a 16-byte boundary: the whole slice goes
    through k_quantize's element-wise loads."""
    from torch_cgx_amd import _C
    x = _input(n, dtype, bits)
    buf = torch.zeros(n + 9, dtype=dtype, device=_dev())
    assert buf.data_ptr() % 16 == 0
    buf[1:1 + n] = x.to(_dev())
    for seed in SEEDS:
        want = golden.quantize(x, bits, bucket,
                               rand=golden.stochastic_rand(seed, n))
        got = _C.quantize(buf[1:1 + n], bits, bucket, True, seed).cpu()
        _assert_same_bytes(got, want, (n, bucket, bits, dtype, seed))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", EF_SHAPES)
def test_generic_kernel_error_feedback(dtype, bits, n, bucket):
    """Error feedback under stochastic rounding: the bytes and the updated
    residual are the model's."""
    from torch_cgx_amd import _C
    x = _input(n, dtype, bits)
    torch.manual_seed(n + bits)
    fb0 = (torch.randn(n) * 0.1).to(dtype)
    xg = x.to(_dev())
    for seed in SEEDS:
        fb_gold = fb0.clone()
        want = golden.quantize_ef(x.clone(), fb_gold, bits, bucket,
                                  rand=golden.stochastic_rand(seed, n))
        fb_gpu = fb0.to(_dev())
        got = _C.quantize(xg, bits, bucket, True, seed, False, fb_gpu).cpu()
        _assert_same_bytes(got, want, (n, bucket, bits, dtype, seed))
        assert torch.equal(fb_gpu.cpu(), fb_gold), (n, bucket, bits, seed)
        assert not torch.equal(fb_gold, fb0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", TWO_PASS_SHAPES)
def test_pack_generic_kernel(dtype, bits, n, bucket):
    """bucket % 8 != 0: k_pack_generic, whose packs straddle buckets."""
    _check(_input(n, dtype, bits), bits, bucket)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,bucket", SKIP_SHAPES)
def test_skip_incomplete(dtype, bits, n, bucket):
    """skip_incomplete: the head is rounded stochastically, the raw tail
    draws nothing."""
    _check(_input(n, dtype, bits), bits, bucket, skip=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", WIDE_BITS)
@pytest.mark.parametrize("n,bucket", WIDE_SHAPES)
def test_wide_packs(dtype, bits, n, bucket):
    """5 to 7 bits on one shape per kernel: k_quantize_fast (with its tail),
    k_quantize_sub (with its tail), k_quantize, k_pack_generic."""
    _check(_input(n, dtype, bits), bits, bucket)


@pytest.mark.parametrize("n,bucket", TWIN_SHAPES)
def test_seed_decides_the_bytes(n, bucket):
    """The same seed gives the same bytes, another seed other packed bytes
    and the same meta, and neither gives the deterministic rounding."""
    from torch_cgx_amd import _C
    bits = 4
    xg = _input(n, torch.float32).to(_dev())
    meta = 8 * golden.num_buckets(n, bucket)
    a = _C.quantize(xg, bits, bucket, True, 1).cpu()
    assert torch.equal(a, _C.quantize(xg, bits, bucket, True, 1).cpu())
    b = _C.quantize(xg, bits, bucket, True, 2).cpu()
    det = _C.quantize(xg, bits, bucket, False, 1).cpu()
    assert torch.equal(a[:meta], b[:meta]) and torch.equal(a[:meta],
                                                           det[:meta])
    assert not torch.equal(a[meta:], b[meta:])
    assert not torch.equal(a[meta:], det[meta:])
    assert not torch.equal(b[meta:], det[meta:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,bucket,lo,hi", [
    pytest.param(1536, 512, 512, 1024, id="fast"),
    pytest.param(320, 64, 64, 128, id="sub"),
    pytest.param(4100, 4096, 0, 4096, id="generic"),
    pytest.param(1003, 50, 150, 200, id="two-pass"),
])
def test_constant_bucket_stays_zero(dtype, n, bucket, lo, hi):
    """unit < EPS: a bucket of equal values encodes to level 0 whatever the
    draw, next to buckets that are rounded stochastically."""
    from torch_cgx_amd import _C
    bits = 4
    x = _input(n, dtype)
    x[lo:hi] = x[lo]
    _check(x, bits, bucket)
    got = _C.quantize(x.to(_dev()), bits, bucket, True, 7).cpu()
    meta = 2 * golden.num_buckets(n, bucket) * golden.elem_size(dtype)
    levels = golden.unpack_levels(got[meta:].numpy(), n, bits)
    assert not levels[lo:hi].any()
    assert levels[:lo].any() or levels[hi:].any()


# ---------------------------------------------------------------------------
# several slices in one launch: the slice index of the key, one seed per group
# ---------------------------------------------------------------------------
def _route(xs, bits, buckets, skip=False):
    """The router's plan for these tensors (the output addresses play no part
    in routing)."""
    from torch_cgx_amd import _C
    return _C.route_quantize([
        (x.data_ptr(), 0x1000 * (i + 1), 0, x.numel(), b, bk, skip)
        for i, (x, b, bk) in enumerate(zip(xs, bits, buckets))])


def _placement(groups, ptr):
    """(group ordinal, index in group) of the slice's body desc and of its
    tail desc (None without one)."""
    from torch_cgx_amd import _C
    body = tail = None
    for k, (_, _, descs, _, _, _) in enumerate(groups):
        for j, d in enumerate(descs):
            if d[0] != ptr:
                continue
            if d[5] & _C.FLAG_TAIL_ONLY:
                assert tail is None
                tail = (k, j)
            else:
                assert body is None
                body = (k, j)
    assert body is not None
    return body, tail


def _slice_rand(groups, ptr, n, bucket, seed):
    """The model's rand for one slice of a quantize_slices call: the body
    desc's (seed + group ordinal, index in group) for the packs of the full
    buckets, the tail desc's for the packs from there on."""
    body, tail = _placement(groups, ptr)
    npacks = (n + 7) // 8
    p0 = (n // bucket) * bucket // 8 if tail else npacks
    words = [golden.pack_rand_words(seed + body[0], body[1], 0, p0)]
    if tail:
        words.append(golden.pack_rand_words(seed + tail[0], tail[1], p0,
                                            npacks - p0))
    return golden.rand_from_words(np.concatenate(words), n)


def _check_slices(cpu, bits, buckets, seed):
    from torch_cgx_amd import _C
    xs = [x.to(_dev()) for x in cpu]
    assert all(x.data_ptr() % 16 == 0 for x in xs)
    groups = _route(xs, bits, buckets)
    outs = _C.quantize_slices(xs, bits, buckets, True, seed)
    assert len(outs) == len(xs)
    for i, (x, b, bk) in enumerate(zip(cpu, bits, buckets)):
        rand = _slice_rand(groups, xs[i].data_ptr(), x.numel(), bk, seed)
        want = golden.quantize(x, b, bk, rand=rand)
        _assert_same_bytes(outs[i].cpu(), want,
                           (i, x.numel(), b, bk, x.dtype, seed))
    return xs, groups, outs


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dtype,bits", [
    pytest.param(torch.float32, [4, 4, 4, 4], id="fp32-4444"),
    pytest.param(torch.float32, [4, 2, 4, 2], id="fp32-4242"),
    pytest.param(torch.bfloat16, [4, 4, 4, 4], id="bf16-4444"),
])
def test_slices_in_one_launch(dtype, bits, seed):
    from torch_cgx_amd import _C
    cpu = [_input(n, dtype, i) for i, (n, _) in enumerate(MULTI_SLICES)]
    buckets = [bk for _, bk in MULTI_SLICES]
    xs, groups, _ = _check_slices(cpu, bits, buckets, seed)
    if bits == [4, 4, 4, 4]:
        # the placements this case is about: slice 1's body is index 1 of the
        # fast group while its tail is index 0 of the generic group, and the
        # four groups run with four seeds
        assert [(g[0], g[1]) for g in groups] == [
            (4, _C.KIND_FAST), (4, _C.KIND_GENERIC), (4, _C.KIND_TWO_PASS),
            (4, _C.KIND_SUB)]
        assert _placement(groups, xs[0].data_ptr()) == ((0, 0), None)
        assert _placement(groups, xs[1].data_ptr()) == ((0, 1), (1, 0))
        assert _placement(groups, xs[2].data_ptr()) == ((3, 0), None)
        assert _placement(groups, xs[3].data_ptr()) == ((2, 0), None)


@pytest.mark.parametrize("n,bucket", TWIN_SHAPES)
def test_identical_slices_draw_independent_streams(n, bucket):
    """Two slices with the same values in one launch group differ in the
    slice index alone: each equals its own model bytes, and their packed
    bytes differ."""
    bits = 4
    x = _input(n, torch.float32)
    xs, groups, outs = _check_slices([x, x.clone()], [bits, bits],
                                     [bucket, bucket], 3)
    assert len(groups) == 1
    assert _placement(groups, xs[0].data_ptr()) == ((0, 0), None)
    assert _placement(groups, xs[1].data_ptr()) == ((0, 1), None)
    meta = 8 * golden.num_buckets(n, bucket)
    a, b = outs[0].cpu(), outs[1].cpu()
    assert torch.equal(a[:meta], b[:meta])
    assert not torch.equal(a[meta:], b[meta:])


def test_quantize_slices_deterministic_matches_quantize():
    """The seam itself: with deterministic rounding every slice is the
    single-slice call's bytes."""
    from torch_cgx_amd import _C
    cpu = [_input(n, torch.float32, i) for i, (n, _) in enumerate(MULTI_SLICES)]
    buckets = [bk for _, bk in MULTI_SLICES]
    xs = [x.to(_dev()) for x in cpu]
    outs = _C.quantize_slices(xs, [4, 2, 4, 2], buckets, False, 0)
    for x, out, b, bk in zip(cpu, outs, [4, 2, 4, 2], buckets):
        _assert_same_bytes(out.cpu(), golden.quantize(x, b, bk),
                           (x.numel(), b, bk))
