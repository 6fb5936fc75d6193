"""The backend's p2p collectives with real peers on ONE MI355X.

allgather / gather / scatter / alltoall / alltoall_base are free functions
over a byte `Transport` (csrc/collectives.{h,cc}); ProcessGroupCGX calls them
over RCCL.  `_C.loopback_collective` runs the same functions at world sizes
2-4 through the loopback transport, so their peer loops, slot indexing, root
handling and split arithmetic execute here.  Every value encodes (rank, peer,
index): a misrouted slot cannot compare equal.  These are byte copies, so
every comparison is exact.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

WORLD_SIZES = [2, 3, 4]
DTYPES = [torch.uint8, torch.bfloat16, torch.float32, torch.int64]
NUMELS = [1, 7, 1000]
SENTINEL = 255  # outside the encoded values, exact in every dtype


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _enc(rank, peer, shape, dtype):
    """CPU tensor whose element i is (53*rank + 17*peer + 1 + i) % 251: below
    the sentinel, exact in bf16 and uint8, and for ranks and peers below 4 no
    two (rank, peer) pairs start at the same value."""
    n = 1
    for s in shape:
        n *= s
    v = (torch.arange(n) + 53 * rank + 17 * peer + 1) % 251
    return v.to(dtype).reshape(shape)


def _blank(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype)


def _run(name, ins, outs, **kw):
    """ins[r] / outs[r]: rank r's CPU tensor lists.  Runs the collective on
    device copies, checks the inputs came through unchanged and returns the
    outputs, back on the CPU."""
    from torch_cgx_amd import _C
    d_ins = [[t.to(_dev()) for t in ts] for ts in ins]
    d_outs = [[t.to(_dev()) for t in ts] for ts in outs]
    _C.loopback_collective(name, d_ins, d_outs, **kw)
    for r, (ts, d_ts) in enumerate(zip(ins, d_ins)):
        for p, (t, d_t) in enumerate(zip(ts, d_ts)):
            assert torch.equal(d_t.cpu(), t), (name, "input changed", r, p)
    return [[t.cpu() for t in ts] for ts in d_outs]


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_allgather(ws, dtype, n):
    ins = [[_enc(r, 0, (n,), dtype)] for r in range(ws)]
    outs = [[_blank((n,), dtype) for _ in range(ws)] for _ in range(ws)]
    got = _run("allgather", ins, outs)
    for r in range(ws):
        for p in range(ws):
            assert torch.equal(got[r][p], ins[p][0]), (r, p)


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_alltoall(ws, dtype, n):
    ins = [[_enc(r, p, (n,), dtype) for p in range(ws)] for r in range(ws)]
    outs = [[_blank((n,), dtype) for _ in range(ws)] for _ in range(ws)]
    got = _run("alltoall", ins, outs)
    for r in range(ws):
        for p in range(ws):
            assert torch.equal(got[r][p], ins[p][r]), (r, p)


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("last_root", [False, True])
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_gather(ws, last_root, dtype, n):
    root = ws - 1 if last_root else 0
    ins = [[_enc(r, root, (n,), dtype)] for r in range(ws)]
    outs = [[_blank((n,), dtype) for _ in range(ws)] if r == root else []
            for r in range(ws)]
    got = _run("gather", ins, outs, root=root)
    for r in range(ws):
        assert len(got[r]) == (ws if r == root else 0)
    for p in range(ws):
        assert torch.equal(got[root][p], ins[p][0]), p


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("last_root", [False, True])
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_scatter(ws, last_root, dtype, n):
    root = ws - 1 if last_root else 0
    ins = [[_enc(root, p, (n,), dtype) for p in range(ws)] if r == root
           else [] for r in range(ws)]
    outs = [[_blank((n,), dtype)] for _ in range(ws)]
    got = _run("scatter", ins, outs, root=root)
    for r in range(ws):
        assert torch.equal(got[r][0], ins[root][r]), r


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_alltoall_base_even(ws, dtype, k):
    """Empty splits: rank r's k-element slice p goes to slice r of rank p."""
    ins = [[torch.cat([_enc(r, p, (k,), dtype) for p in range(ws)])]
           for r in range(ws)]
    outs = [[_blank((ws * k,), dtype)] for _ in range(ws)]
    got = _run("alltoall_base", ins, outs)
    for r in range(ws):
        expected = torch.cat([ins[p][0][r * k:(r + 1) * k]
                              for p in range(ws)])
        assert torch.equal(got[r][0], expected), r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws", WORLD_SIZES)
def test_alltoall_base_splits(ws, dtype):
    """Explicit row splits on [rows, 5] tensors: rank r sends S[r][p] =
    (r + 2p) % 3 rows to p, so splits are unequal, some are zero (every self
    slot among them) and uint8 slices start at odd byte offsets."""
    S = [[(r + 2 * p) % 3 for p in range(ws)] for r in range(ws)]
    in_splits = [S[r] for r in range(ws)]
    out_splits = [[S[p][r] for p in range(ws)] for r in range(ws)]
    # blocks[r][p]: the rows rank r sends to rank p
    blocks = [[_enc(r, p, (S[r][p], 5), dtype) for p in range(ws)]
              for r in range(ws)]
    ins = [[torch.cat(blocks[r])] for r in range(ws)]
    outs = [[_blank((sum(out_splits[r]), 5), dtype)] for r in range(ws)]
    got = _run("alltoall_base", ins, outs, in_splits=in_splits,
               out_splits=out_splits)
    for r in range(ws):
        expected = torch.cat([blocks[p][r] for p in range(ws)])
        assert torch.equal(got[r][0], expected), r


def test_bad_calls_raise_before_any_rank_starts():
    """Unknown names, list lengths that do not fit the world size and
    tensors off the device are refused on the host."""
    from torch_cgx_amd import _C

    def t():
        return torch.zeros(4, device=_dev())

    with pytest.raises(RuntimeError, match="unknown collective"):
        _C.loopback_collective("allscatter", [[t()], [t()]], [[t()], [t()]])
    with pytest.raises(RuntimeError, match="output tensors"):  # 1 of 2 slots
        _C.loopback_collective("allgather", [[t()], [t()]], [[t()], [t()]])
    with pytest.raises(RuntimeError, match="output tensors"):  # non-root list
        _C.loopback_collective("gather", [[t()], [t()]],
                               [[t(), t()], [t(), t()]])
    with pytest.raises(RuntimeError, match="per rank"):
        _C.loopback_collective("alltoall_base", [[t()], [t()]], [[t()]])
    with pytest.raises(RuntimeError, match="CUDA contiguous"):
        _C.loopback_collective("alltoall_base", [[t()], [torch.zeros(4)]],
                               [[t()], [t()]])


def test_alltoall_base_indivisible_raises():
    """A tensor the world size does not divide, and no splits: a host-side
    error on every rank, raised to the caller instead of blocking."""
    from torch_cgx_amd import _C
    ins = [[torch.zeros(7, device=_dev())] for _ in range(2)]
    outs = [[torch.zeros(7, device=_dev())] for _ in range(2)]
    with pytest.raises(RuntimeError, match="not divisible by world size"):
        _C.loopback_collective("alltoall_base", ins, outs)
