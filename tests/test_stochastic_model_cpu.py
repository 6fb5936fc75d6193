"""The host model of the stochastic-rounding hash (golden.pack_rand_words /
golden.stochastic_rand), without a GPU: known answers, the key layout, the
quality of the byte draws the kernels consume, and the rounding bias they
imply.  tests/test_gpu_stochastic.py holds the kernels to this model byte for
byte; this file holds the model to published numbers and to its contract."""

import numpy as np
import pytest
import torch

from torch_cgx_amd.ops import golden

# Engine::Engine: seed_ = 0x9E37.. ^ (0xD1B5.. * (rank + 1)), here rank 0
ENGINE_SEED0 = 0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03
SEEDS = [0, 1, ENGINE_SEED0, ENGINE_SEED0 + 1]


def test_splitmix64_known_answers():
    # rand_pack(0, k) is the k-th output of splitmix64 started at state 0
    # (the published sequence, e.g. the xoshiro seeding reference)
    words = golden.pack_rand_words(0, 0, 1, 3)
    assert words.dtype == np.uint64
    assert [int(w) for w in words] == [
        0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # first_pack offsets the key, nothing else
    assert int(golden.pack_rand_words(0, 0, 3, 1)[0]) == 0x06C45D188009454F


def _mix(z):
    """splitmix64's finalizer on a Python int."""
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_key_layout():
    m = (1 << 64) - 1
    # slice 1, pack 0 is raw key 1 << 44
    for seed in SEEDS:
        raw = _mix((seed + (1 << 44) * 0x9E3779B97F4A7C15) & m)
        assert int(golden.pack_rand_words(seed, 1, 0, 1)[0]) == raw
    # pack p of slice s is raw key (s << 44) | p, at a pack index above 2^32
    raw = _mix((7 + ((3 << 44) | ((1 << 33) + 5)) * 0x9E3779B97F4A7C15) & m)
    assert int(golden.pack_rand_words(7, 3, (1 << 33) + 5, 1)[0]) == raw
    # the slice index changes every pack's word
    a = golden.pack_rand_words(0, 0, 0, 4096)
    b = golden.pack_rand_words(0, 1, 0, 4096)
    assert (a != b).all()
    assert len(np.unique(np.concatenate([a, b]))) == 8192


def test_seed_wraps_mod_2_64():
    a = golden.pack_rand_words(-1, 2, 5, 64)
    b = golden.pack_rand_words(2 ** 64 - 1, 2, 5, 64)
    assert np.array_equal(a, b)
    assert torch.equal(golden.stochastic_rand(-1, 100),
                       golden.stochastic_rand(2 ** 64 - 1, 100))


def test_stochastic_rand_is_rand_lane():
    n = 29  # a partial last pack
    words = golden.pack_rand_words(5, 2, 0, 4)
    r = golden.stochastic_rand(5, n, slice_idx=2)
    assert r.dtype == torch.float32 and r.shape == (n,)
    for i in range(n):
        byte = (int(words[i // 8]) >> (8 * (i % 8))) & 0xFF
        assert r[i].item() == byte / 256
    assert golden.stochastic_rand(5, 0).numel() == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_byte_uniformity(seed):
    """Chi-square of each byte position over 2^17 packs against uniform on 256
    values, below 348: the 99.99% point of chi-square with 255 degrees of
    freedom (Wilson-Hilferty: 255 * (1 - 2/2295 + 3.719 * sqrt(2/2295))^3).
    The inputs are fixed, so the figures are too; measured per seed (min to
    max over the 8 positions): seed 0: 229 to 299; seed 1: 237 to 286;
    engine seed: 232 to 308; engine seed + 1: 203 to 280."""
    npacks = 1 << 17
    words = golden.pack_rand_words(seed, 0, 0, npacks)
    expected = npacks / 256
    chis = []
    for j in range(8):
        by = ((words >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.int64)
        counts = np.bincount(by, minlength=256)
        chis.append(float(((counts - expected) ** 2).sum() / expected))
    print(f"seed {seed:#x}: chi-square per byte position "
          f"{[round(c) for c in chis]}")
    assert max(chis) < 348, chis


@pytest.mark.parametrize("seed", SEEDS[:3])
def test_consecutive_seeds_are_unrelated(seed):
    """The engine hands launch k the seed s + k.  Bytes of seeds s and s + 1 at
    the same packs agree as often as independent uniform bytes would: within
    5 sigma of 1/256 over 2^20 bytes (sigma 0.000061; measured 0.003785,
    0.003848 and 0.003882 against 1/256 = 0.003906)."""
    npacks = 1 << 17
    a = golden.pack_rand_words(seed, 0, 0, npacks).view(np.uint8)
    b = golden.pack_rand_words(seed + 1, 0, 0, npacks).view(np.uint8)
    nbytes = 1 << 20
    assert a.size == nbytes
    p = 1 / 256
    sigma = (p * (1 - p) / nbytes) ** 0.5
    frac = float((a == b).mean())
    print(f"seed {seed:#x}: equal-byte fraction {frac:.6f} (1/256 = {p:.6f}, "
          f"sigma {sigma:.6f})")
    assert abs(frac - p) < 5 * sigma, (frac, p, sigma)


@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_rounding_bias(bits):
    """A draw in steps of 1/256 rounds a fraction f up with probability
    floor(256 f)/256, so the bias per element lies in (-1/256, 0] of a unit,
    -1/512 on average.  Measured mean bias over seeds 0..255 on these inputs:
    -0.0015 (1 bit), -0.0021 (2), -0.0015 (4), -0.0017 (8); the sampling
    error of the mean of 2^20 draws is about 0.0004."""
    n, bucket = 4096, 64
    torch.manual_seed(bits)
    x = torch.randn(n)
    meta = golden.compute_meta(x, bits, bucket)
    unit = meta[0::2].double().repeat_interleave(bucket)
    bmin = meta[1::2].double().repeat_interleave(bucket)
    top = float((1 << bits) - 1)
    # where an unbiased rounding would land, on average: the exact position
    pos = torch.clamp((x.double() - bmin) / unit, max=top).numpy()
    acc = np.zeros(n, dtype=np.float64)
    for seed in range(256):
        acc += golden.encode_levels(x, meta, bits, bucket,
                                    rand=golden.stochastic_rand(seed, n))
    bias = float((acc / 256 - pos).mean())
    print(f"bits {bits}: mean rounding bias {bias:.5f} units")
    assert -1 / 256 < bias < 0, bias


@pytest.mark.parametrize("dtype",
                         [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,bucket", [(1000, 512), (1025, 64), (7, 512),
                                      (1024, 512)])
def test_skip_incomplete_takes_a_rand_tensor(dtype, n, bucket):
    torch.manual_seed(n)
    x = torch.randn(n).to(dtype)
    rand = golden.stochastic_rand(3, n)
    nq = n // bucket * bucket
    out = golden.quantize(x, 4, bucket, rand=rand, skip_incomplete=True)
    assert out.numel() == golden.buffer_size(n, dtype, 4, bucket, True)
    tail = golden._raw_bytes(x[nq:])
    if nq:
        head = golden.quantize(x[:nq], 4, bucket, rand=rand[:nq])
        assert torch.equal(out[:head.numel()], head)
        assert head.numel() + tail.numel() == out.numel()
        # the head is really rounded stochastically
        assert not torch.equal(head, golden.quantize(x[:nq], 4, bucket))
    assert torch.equal(out[out.numel() - tail.numel():], tail)
    # a scalar rand is unchanged
    assert torch.equal(
        golden.quantize(x, 4, bucket, rand=0.5, skip_incomplete=True),
        golden.quantize(x, 4, bucket, skip_incomplete=True))


@pytest.mark.parametrize("dtype",
                         [torch.float32, torch.float16, torch.bfloat16])
def test_encode_levels_accepts_the_rand_tensor(dtype):
    """Levels with the model's rand are within one of the deterministic ones,
    and differ from them: the tensor is used, element by element."""
    n, bits, bucket = 1003, 4, 50
    torch.manual_seed(1)
    x = torch.randn(n).to(dtype)
    meta = golden.compute_meta(x, bits, bucket)
    det = golden.encode_levels(x, meta, bits, bucket).astype(np.int64)
    sto = golden.encode_levels(
        x, meta, bits, bucket,
        rand=golden.stochastic_rand(9, n)).astype(np.int64)
    assert np.abs(sto - det).max() == 1
