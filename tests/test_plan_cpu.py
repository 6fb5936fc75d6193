"""Chunk planning (csrc/plan.h plan_bucket / plan_chunk) on the CPU: which
bytes of a bucket travel in which chunk, and which slices of a chunk belong
to which rank.

The Python mirrors are the oracle: partition.partition, partition.layer_slices
and golden.buffer_size.  Layers lie back to back from byte offset 0, so every
`data` the seams return is a byte offset into the bucket."""

import pytest
import torch

from torch_cgx_amd import _C
from torch_cgx_amd.ops import golden
from torch_cgx_amd.parallel import partition as P

LAYERS = [1000, 513, 2048, 31, 7]
CFGS = [(4, 512), (8, 64), (2, 1024), (32, 512), (4, 512)]
MIN_ELEMS = 16
BIG = 64 << 20
DTYPES = [torch.float32, torch.float16]
WORLDS = [1, 2, 3, 4, 8]
# layers 0..2 are compressible: elements [0, 3561)
N_COMP = 3561


def _es(dtype):
    return golden.elem_size(dtype)


def _plan_bucket(dtype, fusion_bytes, fake_ratio=1.0, dummy=False):
    uncomp, chunks = _C.plan_bucket(LAYERS, CFGS, dtype, fusion_bytes,
                                    MIN_ELEMS, fake_ratio, dummy)
    return ([tuple(u) for u in uncomp],
            [[tuple(v) for v in c] for c in chunks])


def _layer_cfg_at(elem):
    pos = 0
    for n, cfg in zip(LAYERS, CFGS):
        if pos <= elem < pos + n:
            return cfg
        pos += n
    raise AssertionError(elem)


def _check_tiling(chunks, es):
    """The chunks cover the compressible elements exactly once, in order, and
    every piece carries the config of the layer it lies in."""
    pos = 0
    for chunk in chunks:
        assert chunk
        for off, numel, bits, bucket in chunk:
            assert off == pos * es and numel > 0
            assert (bits, bucket) == _layer_cfg_at(pos)
            assert (bits, bucket) == _layer_cfg_at(pos + numel - 1)
            pos += numel
    assert pos == N_COMP


def _sizes(chunks):
    return [[v[1] for v in c] for c in chunks]


# ---------------------------------------------------------------------------
# plan_bucket
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bucket_split(dtype):
    es = _es(dtype)
    # layer 3 (bits 32) and layer 4 (7 <= 16 elements) are adjacent: one range
    for fusion in (2048, BIG):
        uncomp, _ = _plan_bucket(dtype, fusion)
        assert uncomp == [(N_COMP * es, 38)]
    uncomp, chunks = _plan_bucket(dtype, BIG, dummy=True)
    assert uncomp == [(0, 3599)]
    assert chunks == []


def test_fusion_fp32():
    # fusion_elems = 2048 / 4 = 512
    _, chunks = _plan_bucket(torch.float32, 2048)
    assert _sizes(chunks) == [[512], [488], [512], [1]] + [[512]] * 4
    cfgs = [c[0][2:] for c in chunks]
    assert cfgs == [CFGS[0]] * 2 + [CFGS[1]] * 2 + [CFGS[2]] * 4
    _check_tiling(chunks, 4)


def test_fusion_fp16():
    # fusion_elems = 2048 / 2 = 1024; 1000 + 513 overflows it
    _, chunks = _plan_bucket(torch.float16, 2048)
    assert _sizes(chunks) == [[1000], [513], [1024], [1024]]
    _check_tiling(chunks, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_one_chunk(dtype):
    es = _es(dtype)
    _, chunks = _plan_bucket(dtype, BIG)
    assert chunks == [[(0, 1000, 4, 512), (1000 * es, 513, 8, 64),
                       (1513 * es, 2048, 2, 1024)]]
    _check_tiling(chunks, es)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fusion", [2048, BIG])
def test_fake_ratio(dtype, fusion):
    _, full = _plan_bucket(dtype, fusion)
    _, trimmed = _plan_bucket(dtype, fusion, fake_ratio=0.5)
    assert len(trimmed) == len(full)
    for chunk, cut in zip(full, trimmed):
        total = sum(v[1] for v in chunk)
        keep = max(16, int(total * 0.5))
        want = []
        for off, numel, bits, bucket in chunk:
            if keep <= 0:
                break
            want.append((off, min(numel, keep), bits, bucket))
            keep -= want[-1][1]
        assert cut == want
        assert cut[0][0] == chunk[0][0]  # the error-feedback key's pointer


# ---------------------------------------------------------------------------
# plan_chunk
# ---------------------------------------------------------------------------
def _all_chunks():
    out = []
    for dtype in DTYPES:
        for fusion in (2048, BIG):
            for ratio in (1.0, 0.5):
                _, chunks = _plan_bucket(dtype, fusion, fake_ratio=ratio)
                out += [(dtype, c) for c in chunks]
    return out


CHUNKS = _all_chunks()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("ws", WORLDS)
def test_chunk_plan(ws, skip):
    assert any(sum(v[1] for v in c) == 1 for _, c in CHUNKS)
    for dtype, chunk in CHUNKS:
        es = _es(dtype)
        numels = [v[1] for v in chunk]
        n = sum(numels)
        view_pos = [sum(numels[:i]) for i in range(len(chunk))]
        offs, szs, comp, rs = _C.plan_chunk(chunk, dtype, ws, skip)
        want_offs, want_szs = P.partition(n, ws, 0, numels, dtype)
        assert (list(offs), list(szs)) == (want_offs, want_szs)
        assert len(rs) == ws and len(comp) == ws
        for r in range(ws):
            want = P.layer_slices(numels, offs[r], szs[r])
            assert len(rs[r]) == len(want)
            coff = 0
            for got, (li, lo, cnt) in zip(rs[r], want):
                off, m, bits, bucket, comp_off, sk, fb_off = got
                # chunk element `lo` lies (lo - view_pos) elements into view li
                voff, _, vbits, vbucket = chunk[li]
                assert off == voff + (lo - view_pos[li]) * es
                assert (m, bits, bucket, sk) == (cnt, vbits, vbucket, skip)
                assert fb_off == lo
                assert comp_off == coff
                coff += golden.buffer_size(cnt, dtype, bits, bucket, skip)
            assert comp[r] == coff
            if szs[r] == 0:
                assert rs[r] == [] and comp[r] == 0
        if ws == 1:
            assert [(s[0], s[1]) for s in rs[0]] == [(v[0], v[1])
                                                     for v in chunk]
        if n == 1 and ws == 8:
            # a 1-element chunk: seven ranks own nothing
            assert sorted(szs) == [0] * 7 + [1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_plan_contiguous_offsets(dtype):
    # views back to back in memory: byte_off / es is the chunk element offset
    es = _es(dtype)
    _, (chunk,) = _plan_bucket(dtype, BIG)
    numels = [v[1] for v in chunk]
    for ws in WORLDS:
        offs, szs, _, rs = _C.plan_chunk(chunk, dtype, ws, False)
        for r in range(ws):
            assert [(s[0] // es, s[1]) for s in rs[r]] == [
                (lo, cnt) for _, lo, cnt in P.layer_slices(numels, offs[r],
                                                           szs[r])]


def test_empty_chunk():
    offs, szs, comp, rs = _C.plan_chunk([(0, 0, 4, 512)], torch.float32, 4,
                                        False)
    assert (list(offs), list(szs), list(comp), list(rs)) == ([], [], [], [])
