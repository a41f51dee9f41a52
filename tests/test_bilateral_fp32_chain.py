"""The bilateral filter's fp32 tap chain (tsdf_amd/csrc/bilateral_chain.hpp): interior waves of the staged 15 x 15 kernel run a half
column of taps as fp32 fmas where chain_certified proves that this rounds like the reference's float/double expression, and redo it
in double elsewhere.

CPU (no GPU): the kernel's own tap expressions and test, through tsdf_selftest_bilateral_chain_taps / _image -- every certified tap
gives identical bits, constructed double-rounding cases are rejected, and the host run of the whole chain equals the oracle.
GPU: the filter bit for bit against the oracle at the smallest sizes with interior + rim waves (48 x 40) and rim waves only (33 x 19)."""
import ctypes as C

import numpy as np
import pytest

import tsdf_amd
from tsdf_amd import _capi

SIGMAS = (30.0, 4.5)                                   # the pipeline's filter: 15 x 15 taps, smallest weight 1.9e-34
# its smallest tap weight: the float product of the smallest entries of the two tables
MIN_WEIGHT = np.float32(np.exp(np.float32(-98.0) * (np.float32(1.0) / np.float32(20.25)))) * \
    np.float32(np.exp(np.float32(-65535.0) * (np.float32(1.0) / np.float32(900.0))))


def run_taps(w, v4, s):
    w = np.ascontiguousarray(w, np.float32)
    v4 = np.ascontiguousarray(v4, np.uint32)
    s = np.ascontiguousarray(s, np.float32)
    n = w.size
    assert v4.size == n and s.size == n
    f32, f64, ok = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.uint8)
    rc = _capi.lib.tsdf_selftest_bilateral_chain_taps(n, w.ctypes.data, v4.ctypes.data, s.ctypes.data, f32.ctypes.data, f64.ctypes.data,
                                                      ok.ctypes.data)
    assert rc == 0, _capi.lib.tsdf_last_error()
    # the reference's expression on its own: the double product is exact (24 + 18 bits), one rounding of the sum, one narrowing
    assert np.array_equal(f64.view(np.uint32), (w.astype(np.float64) * v4.astype(np.float64) + s.astype(np.float64)).astype(np.float32).view(np.uint32))
    return f32.view(np.uint32), f64.view(np.uint32), ok.astype(bool)


def run_image(img, sigmas=SIGMAS):
    h, w = img.shape
    out = np.empty_like(img)
    counts = (C.c_uint64 * 4)()
    rc = _capi.lib.tsdf_selftest_bilateral_chain_image(sigmas[0], sigmas[1], img.ctypes.data, 8 * img.itemsize, w, h, out.ctypes.data, counts)
    assert rc == 0, _capi.lib.tsdf_last_error()
    return out, list(counts)


def random_weights(rng, n):
    # mantissas uniform, exponents uniform over 2^-120 ... 1
    w = (rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(-120, 0, n))).astype(np.float32)
    return np.minimum(w, np.float32(1.0))


def random_v4(rng, n):
    v = rng.randint(0, 65536, n).astype(np.uint32)
    pick = rng.randint(0, 8, n)
    v[pick == 0] = 0
    v[pick == 1] = 1
    v[pick == 2] = 65535
    return 4 * v


def tap_families():
    """(name, w, v4, s, smallest share of the family the test must certify): some millions of taps in all."""
    rng = np.random.RandomState(0xB11A)
    n = 1 << 20
    w, v4 = random_weights(rng, n), random_v4(rng, n)
    # sums anywhere in the range
    yield "random", w, v4, (rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(-118, 40, n))).astype(np.float32), 0.05
    # sums within 2^+-24 of the product: what the filter's chain mostly sees
    w, v4 = random_weights(rng, n), random_v4(rng, n)
    p = np.maximum(w.astype(np.float64) * np.maximum(v4, 4), 2.0 ** -118)
    s = np.clip(p * rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(-24, 25, n)), 2.0 ** -118, 2.0 ** 39).astype(np.float32)
    yield "near the product", w, v4, s, 0.5
    # sums that put w v4 + s within an ulp of a float midpoint: s = a midpoint - the product, rounded, and its neighbours
    w, v4 = random_weights(rng, n), random_v4(rng, n)
    p = w.astype(np.float64) * v4
    f = np.clip(np.maximum(p, 2.0 ** -110) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(0, 30, n)), 2.0 ** -110, 2.0 ** 39).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    s0 = np.maximum(mid - p, 0.0).astype(np.float32)
    for name, s in (("midpoint", s0), ("midpoint + ulp", np.nextafter(s0, np.float32(np.inf))),
                    ("midpoint - ulp", np.nextafter(s0, np.float32(0.0)))):
        s = np.where(s < np.float32(2.0 ** -118), np.float32(0.0), s).astype(np.float32)
        yield name, w, v4, s, 0.3
    # an empty sum, and a sum that is the filter's smallest weight (and the smallest the staged kernel admits)
    w, v4 = random_weights(rng, n), random_v4(rng, n)
    yield "s = 0", w, v4, np.zeros(n, np.float32), 1.0
    yield "s = smallest weight", w, v4, np.full(n, MIN_WEIGHT, np.float32), 0.0
    yield "s = 2^-120", w, v4, np.full(n, 2.0 ** -120, np.float32), 0.0
    # v4 in {0, 4, 4 * 65535} against every exponent of w and s
    ew, es = np.meshgrid(np.arange(-120, 1), np.arange(-120, 40))
    m = rng.uniform(1.0, 2.0, ew.size)
    for v in (0, 4, 4 * 65535):
        yield "v4 = %d" % v, np.minimum(m * np.exp2(ew.ravel()), 1.0).astype(np.float32), np.full(ew.size, v, np.uint32), \
            (rng.uniform(1.0, 2.0, ew.size) * np.exp2(es.ravel())).astype(np.float32), 0.1
    # zero weights
    yield "w = 0", np.zeros(n, np.float32), random_v4(rng, n), (rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(-118, 40, n))).astype(np.float32), 0.0


def test_certified_taps_round_like_the_double_expression():
    assert 1.8e-34 < MIN_WEIGHT < 2.0e-34
    total = certified = 0
    for name, w, v4, s, min_share in tap_families():
        f32, f64, ok = run_taps(w, v4, s)
        bad = ok & (f32 != f64)
        assert not bad.any(), "%s: %d certified taps differ, first w=%r v4=%d s=%r" % (
            name, int(bad.sum()), w[bad][0], v4[bad][0], s[bad][0])
        assert ok.mean() >= min_share, "%s: only %.3f of the taps certified" % (name, ok.mean())
        total += ok.size
        certified += int(ok.sum())
    assert total > 8000000 and certified > total // 2
    # a zero weight or a zero intensity leaves the sum alone in both forms, certified or not
    s = np.float32([0.0, 1.0, 3.5e7, 2.0 ** -120])
    for w, v4 in ((np.zeros(4, np.float32), np.full(4, 4 * 65535, np.uint32)), (np.full(4, 0.37, np.float32), np.zeros(4, np.uint32))):
        f32, f64, _ = run_taps(w, v4, s)
        assert np.array_equal(f32, s.view(np.uint32)) and np.array_equal(f64, s.view(np.uint32))


def test_constructed_double_roundings_are_rejected():
    """w = 2^a (2^m + 1), v4 = 4 (2^m - 1): the product is 2^(a+2) (2^2m - 1), one bit minus one bit 2m places below.  With the upper bit
    half an ulp of s and an odd mantissa of s, w v4 + s lies 2^-(2m + 24) relative below a float midpoint: the double rounds it onto the
    midpoint and the narrowing then rounds to even, upwards, while the single rounding goes down."""
    w, v4, s = [], [], []
    rng = np.random.RandomState(7)
    for m in (15, 16):
        for k in range(-70, 40):                                   # exponent of s
            a = k - 24 - 2 * m - 2                                 # 2^(a + 2 + 2m) = ulp(s) / 2
            for mant in rng.randint(0, 1 << 22, 40) * 2 + 1:       # odd mantissas
                w.append(np.ldexp(float((1 << m) + 1), a))
                v4.append(4 * ((1 << m) - 1))
                s.append(np.ldexp(1.0 + mant * 2.0 ** -23, k))
    w, v4, s = np.float32(w), np.uint32(v4), np.float32(s)
    assert np.array_equal(w.astype(np.float64), np.float64([float(x) for x in w])) and w.min() >= 2.0 ** -120 and w.max() <= 1.0
    f32, f64, ok = run_taps(w, v4, s)
    assert np.array_equal(f32, s.view(np.uint32))                  # one rounding: below the midpoint, down
    assert np.array_equal(f64, s.view(np.uint32) + 1)              # two roundings: onto the midpoint, then to even
    assert not ok.any()


# ---- images: (width, height) 48 x 40 = the smallest with interior waves (a 16-wide tile whose 7-pixel apron is inside the image)
# as well as rim waves; 33 x 19 = rim waves only
SHAPES = [(48, 40), (33, 19)]
CONTENTS = ["constant", "random", "ramp_with_zero_band", "planes_500_60000", "full_with_single_zeros"]


def make_image(content, shape, dtype):
    w, h = shape
    top = np.iinfo(dtype).max
    rng = np.random.RandomState(w * 100 + h)
    if content == "constant":
        img = np.full((h, w), 1234 if dtype == np.uint16 else 77, dtype)
    elif content == "random":
        img = rng.randint(0, top + 1, (h, w)).astype(dtype)
    elif content == "ramp_with_zero_band":
        xx, yy = np.meshgrid(np.arange(w), np.arange(h))
        img = ((800 + 9 * xx + 5 * yy) if dtype == np.uint16 else (40 + 2 * xx + yy)).astype(dtype)
        img[h // 2 - 2:h // 2 + 1, :] = 0
    elif content == "planes_500_60000":
        near, far = (500, 60000) if dtype == np.uint16 else (2, 250)
        img = np.full((h, w), near, dtype)
        img[:, w // 2:] = far                                      # (48 wide: the edge runs through the interior tile, columns 16 .. 31)
    else:
        img = np.full((h, w), top, dtype)
        img[rng.randint(0, h, 12), rng.randint(0, w, 12)] = 0
        img[h // 2, w // 2] = 0
    return np.ascontiguousarray(img)


_expected = {}


def expected(oracle, content, shape, dtype):
    """The oracle's filtered image, computed once per case and shared by the CPU and GPU tests."""
    key = (content, shape, np.dtype(dtype).name)
    if key not in _expected:
        img = make_image(content, shape, dtype)
        fn = oracle.bilateral_u16 if dtype == np.uint16 else oracle.bilateral_u8
        exp = fn(img, shape[0], shape[1], *SIGMAS)
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("content", CONTENTS)
def test_host_chain_equals_oracle(oracle, content, shape, dtype):
    img = make_image(content, shape, dtype)
    out, counts = run_image(img)
    assert np.array_equal(out, expected(oracle, content, shape, dtype).reshape(out.shape))
    # interior waves: 48 x 40 has the tile column 16 .. 31 with wave rows 8 .. 28; 33 x 19 has none
    assert counts[0] == (6 * 30 if shape == (48, 40) else 0) and counts[2] == 64 * counts[0]
    if content == "constant":
        assert counts[1] == 0 and counts[3] == 0
    if content == "planes_500_60000" and dtype == np.uint16 and shape == (48, 40):
        assert counts[1] > 0, "the 500 mm / 60 000 mm edge must force the fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("content", CONTENTS)
def test_gpu_filter_equals_oracle(oracle, content, shape, dtype):
    img = make_image(content, shape, dtype)
    if content == "planes_500_60000" and dtype == np.uint16 and shape == (48, 40):
        assert run_image(img)[1][1] > 0                            # the CPU certificate: this very image takes the fallback
    got = img.copy()
    tsdf_amd.BilateralFilter(*SIGMAS).filter(got, shape[0], shape[1])
    assert np.array_equal(got, expected(oracle, content, shape, dtype).reshape(got.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("content", CONTENTS)
def test_gpu_tile_maxima_unchanged(oracle, content, shape):
    import torch
    w, h = shape
    img = make_image(content, shape, np.uint16)
    exp = expected(oracle, content, shape, np.uint16).reshape(h, w)
    src = torch.from_numpy(img.view(np.int16).copy()).cuda()
    dst = torch.empty_like(src)
    tx, ty = (w + 15) // 16, (h + 15) // 16
    tmax = torch.full((ty * tx,), -1, dtype=torch.int16, device="cuda")
    tsdf_amd.BilateralFilter(*SIGMAS).filter_device(src.data_ptr(), dst.data_ptr(), w, h, bits=16,
                                                    stream=torch.cuda.current_stream().cuda_stream, tile_max_ptr=tmax.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().view(np.uint16).reshape(h, w), exp)
    want = np.array([[exp[j * 16:(j + 1) * 16, i * 16:(i + 1) * 16].max() for i in range(tx)] for j in range(ty)], np.uint16)
    assert np.array_equal(tmax.cpu().numpy().view(np.uint16).reshape(ty, tx), want)
