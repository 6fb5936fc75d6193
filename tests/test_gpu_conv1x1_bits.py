"""The three native 1x1-convolution GEMMs give the bits they gave before their
main loop, dispatch and routing were merged.

Every shape of the SHAPES lists of test_gpu_conv1x1_bn.py, _bwd.py and _wrw.py
(together they reach every instantiation of the kernels, a one-pixel image,
ragged row tails and a capped grid) is run on inputs from a seeded CPU
generator, and the SHA-256 of each output's memory is held against
tests/golden/conv1x1_bits.json.  The kernels have no atomics and a fixed
order of every sum, so equality is what a refactor owes.

The fixture holds hashes only.  It is what this module prints when run as a
script, `python tests/test_gpu_conv1x1_bits.py > tests/golden/conv1x1_bits.json`,
in a build of the commit whose bits are to be kept; it was taken at the parent
of the commit that added this test (benchmarks/RESULTS.md names it).  A hash
that differs after a change to the kernels means the change altered results:
the cause is to be found, not the fixture rewritten from the changed tree.
"""

import functools
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))

import test_gpu_conv1x1_bn as fwd  # noqa: E402
import test_gpu_conv1x1_bwd as bwd  # noqa: E402
import test_gpu_conv1x1_wrw as wrw  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "conv1x1_bits.json")


def _bf16_cl(shape, g):
    return torch.randn(*shape, generator=g).bfloat16().cuda().contiguous(
        memory_format=torch.channels_last)


def _weight(n, k, g):
    return (torch.randn(n, k, 1, 1, generator=g) / 8.0).bfloat16().cuda()


def _sha(t):
    """SHA-256 of the tensor's dense memory, NHWC for a 4-d one."""
    t = t.detach().cpu()
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1)
    return hashlib.sha256(
        t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _stats(s, seed):
    b, k, n, h, w, wg = s
    g = torch.Generator().manual_seed(seed)
    x = _bf16_cl((b, k, h, w), g)
    wt = _weight(n, k, g)
    y, part = _C.conv1x1_stats(x, wt, wg)
    return {"y": _sha(y), "part": _sha(part)}


def _bwd_data(s, seed):
    b, k, n, h, w, wg = s
    g = torch.Generator().manual_seed(seed)
    dy = _bf16_cl((b, n, h, w), g)
    wt = _weight(n, k, g)
    skip = _bf16_cl((b, k, h, w), g)
    return {"dx": _sha(_C.conv1x1_bwd_data(dy, wt, None, wg)),
            "dx_with_skip": _sha(_C.conv1x1_bwd_data(dy, wt, skip, wg))}


def _wrw(s, seed):
    b, k, n, h, w, wg = s
    g = torch.Generator().manual_seed(seed)
    dy = _bf16_cl((b, n, h, w), g)
    x = _bf16_cl((b, k, h, w), g)
    return {"dw": _sha(_C.conv1x1_wrw(dy, x, wg))}


CASES = {}
for _name, _run, _mod in (("stats", _stats, fwd), ("bwd_data", _bwd_data, bwd),
                          ("wrw", _wrw, wrw)):
    for _s in _mod.SHAPES:
        CASES[f"{_name}-{_mod._ids(_s)}"] = functools.partial(
            _run, _s, 1000 + len(CASES))


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_every_case():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_bits_as_recorded(case):
    got = CASES[case]()
    print(case, got)
    assert got == _golden()[case]


if __name__ == "__main__":
    json.dump({c: CASES[c]() for c in sorted(CASES)}, sys.stdout, indent=1,
              sort_keys=True)
    print()
