"""The comparison scheme of tests/_large_calls.py shown to fail where it should, without a GPU.

No kernel with a deliberately narrowed index can be run on the device (it would read out of bounds), so the scheme is
scaled down instead: the boundary sits at 2^20 bytes (and 2^19), the rules for P are the same, and a stand-in "kernel"
in numpy maps every 4 input bytes to one f32 output.  It is corrupted the three ways a narrowed index corrupts a real
kernel -- the read index wrapped, the write index wrapped (an unwritten sentinel region and an overwritten early one),
one channel's pitch product wrapped -- and the helpers must flag each and name the right first period or channel."""
import numpy as np
import pytest

import _large_calls as lc

B = 1 << 20
BOUNDS = (1 << 19, B)
MARGIN = 1 << 14
UNIT, PIECE = 400, 16          # a unit that carries a factor 25, as 25 600 does: P never divides a power of two
P, TAIL = 11 * UNIT, 4 * 613


def kernel(inp, read_wrap=None, write_wrap=None):
    """out[j] = a float in [1, 2) made of input bytes 4j .. 4j+3.  read_wrap: the byte index is taken mod it on read;
    write_wrap: the output's byte offset is taken mod it on write, over an output filled with the NaN sentinel."""
    n = len(inp) // 4
    idx = 4 * np.arange(n, dtype=np.int64)[:, None] + np.arange(4)
    if read_wrap:
        idx %= read_wrap
    word = inp[idx].astype(np.uint32) @ np.array([1, 1 << 8, 1 << 16, 1 << 24], np.uint32)
    val = ((word & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
    out = np.full(n, lc.F32_SENTINEL, np.uint32).view(np.float32)
    j = np.arange(n, dtype=np.int64)
    if write_wrap:
        j = (4 * j % write_wrap) // 4
    out[j] = val                                     # (later writes win, as they would on the device)
    return out


@pytest.fixture(scope="module")
def shape():
    K = lc.periods_needed(P, UNIT, BOUNDS, MARGIN, PIECE)
    lc.check_tail(TAIL, P, 4, UNIT, 64)
    assert K * P >= B + MARGIN and (K - 1) * P < B + MARGIN
    base = np.random.default_rng(5).integers(0, 256, P, dtype=np.uint8)
    stream = np.concatenate([np.tile(base, K), base[:TAIL]])
    control = kernel(np.concatenate([np.tile(base, 3), base[:TAIL]]))
    per = P // 4
    p0, p1 = control[:per], control[per:2 * per]
    lc.assert_no_alias("input", base, BOUNDS)
    lc.assert_no_alias("output", p1, BOUNDS)
    return K, per, stream, p0, p1


def test_a_correct_result_passes(shape):
    K, per, stream, p0, p1 = shape
    lc.check_periodic("clean", kernel(stream), per, K, p0, p1, 4)
    # the control's own periodic property, as the GPU tests assert it
    lc.check_periodic("control", kernel(np.concatenate([stream[:3 * P], stream[:TAIL]])), per, 3, p0, p1, 4)


def test_works_on_torch_tensors_too(shape):
    torch = pytest.importorskip("torch")
    K, per, stream, p0, p1 = shape
    lc.check_periodic("clean", torch.from_numpy(kernel(stream)), per, K, p0, p1, 4)
    with pytest.raises(lc.Mismatch) as e:
        lc.check_periodic("read", torch.from_numpy(kernel(stream, read_wrap=B)), per, K, p0, p1, 4)
    assert e.value.index == B // P


def test_read_index_wrapped(shape):
    """Wrapped data: the first period that reaches past the boundary is the first bad one, and every later one is bad."""
    K, per, stream, p0, p1 = shape
    with pytest.raises(lc.Mismatch) as e:
        lc.check_periodic("read", kernel(stream, read_wrap=B), per, K, p0, p1, 4)
    first = B // P
    assert B % P and e.value.where == "period" and e.value.index == first and e.value.offset == first * P
    assert e.value.bad == list(range(first, K)) and f"period {first} of {K}" in str(e.value) and hex(first * P) in str(e.value)
    # a wrap at the lower boundary is seen at the lower boundary
    with pytest.raises(lc.Mismatch) as e:
        lc.check_periodic("read", kernel(stream, read_wrap=B // 2), per, K, p0, p1, 4)
    assert e.value.index == (B // 2) // P


def test_write_index_wrapped(shape):
    """The region behind the boundary keeps the sentinel, the start of the buffer is overwritten with later data: period 0
    is the first bad one (it no longer equals the control's), and the unwritten periods are all listed."""
    K, per, stream, p0, p1 = shape
    out = kernel(stream, write_wrap=B)
    assert (out.view(np.uint32)[B // 4:] == lc.F32_SENTINEL).all()
    with pytest.raises(lc.Mismatch) as e:
        lc.check_periodic("write", out, per, K, p0, p1, 4)
    assert e.value.where == "period" and e.value.index == 0 and e.value.offset == 0
    assert set(range(B // P, K)) <= set(e.value.bad) and 1 in e.value.bad and "tail" in str(e.value)
    # only the tail unwritten
    out = kernel(stream)
    out.view(np.uint32)[K * per + 7:] = lc.F32_SENTINEL
    with pytest.raises(lc.Mismatch) as e:
        lc.check_periodic("tail", out, per, K, p0, p1, 4)
    assert e.value.where == "tail" and e.value.offset == K * P and "first at element 7" in str(e.value)


def test_one_channels_pitch_product_wrapped():
    """A bank of slots [N, pitch]: channel c reads its block at (c pitch) mod 2^20 -- another channel's bytes."""
    pitch, hist, N = 4000, 800, 300
    rng = np.random.default_rng(6)
    blocks = rng.integers(0, 256, (lc.GROUP, pitch - hist), dtype=np.uint8)
    slots = np.full((N, pitch), 128, np.uint8)
    slots[:, hist:] = blocks[np.arange(N) % lc.GROUP]
    assert N * pitch >= B + MARGIN
    period = slots[:lc.GROUP]
    lc.assert_no_alias("slots", period, BOUNDS)
    flat = slots.reshape(-1)

    def bank(wrapped=()):
        rows = []
        for c in range(N):
            o = c * pitch % B if c in wrapped else c * pitch
            rows.append(kernel(flat[o + hist:o + pitch]))
        return np.stack(rows)

    want = bank()[:lc.GROUP]
    lc.check_channels("clean", bank(), want, in_pitch=pitch)
    first_past = -(-B // pitch)
    c = first_past + 7
    with pytest.raises(lc.Mismatch) as e:
        lc.check_channels("pitch", bank({c}), want, in_pitch=pitch)
    assert e.value.where == "channel" and e.value.index == c and e.value.bad == [c] and hex(c * pitch) in str(e.value)
    with pytest.raises(lc.Mismatch) as e:
        lc.check_channels("pitch", bank(set(range(first_past, N))), want, in_pitch=pitch)
    assert e.value.index == first_past and e.value.bad == list(range(first_past, N))
    # a wrong channel among the first sixteen is a mismatch with the control bank
    out = bank()
    out[3, 5] = 0.0
    with pytest.raises(lc.Mismatch) as e:
        lc.check_channels("control", out, want)
    assert e.value.index == 3 and 3 + lc.GROUP in e.value.bad


def test_rules_refuse_shapes_that_could_alias():
    with pytest.raises(AssertionError, match="divides the boundary"):
        lc.periods_needed(1 << 12, 16, BOUNDS, MARGIN, PIECE)
    with pytest.raises(AssertionError, match="whole number of units"):
        lc.periods_needed(P + 16, UNIT, BOUNDS, MARGIN, PIECE)
    with pytest.raises(AssertionError, match="DMA pieces"):
        lc.periods_needed(UNIT * 11, UNIT, BOUNDS, MARGIN, 1024)
    # a near-periodic signal: the shifted period equals itself almost everywhere
    near = np.tile(np.arange(8, dtype=np.uint8), P // 8)
    near[::97] += 1
    with pytest.raises(AssertionError, match="differs from itself"):
        lc.assert_no_alias("near-periodic", near, BOUNDS)
    with pytest.raises(AssertionError, match="divides the boundary"):
        lc.assert_no_alias("power of two", np.arange(1 << 10, dtype=np.float32), BOUNDS)
    # tails that are a whole batch, or a whole number of 16 outputs
    for tail in (UNIT, 64 * 3, P):
        with pytest.raises(AssertionError):
            lc.check_tail(tail, P, 4, UNIT, 64)
    # the real shapes (the conditions the GPU tests assert, at their P)
    for Pb, unit in ((41 * 25600, 25600), (68 * 15360, 15360), (4 * 256000, 256000)):
        K = lc.periods_needed(Pb, unit)
        assert K * Pb >= (1 << 32) + (64 << 20) and 1_000_000 < Pb < 1_100_000
    assert lc.periods_needed(68 * 15360, 15360, scale=(4, 5)) * 68 * 15360 * 4 >= ((1 << 32) + (64 << 20)) * 5
