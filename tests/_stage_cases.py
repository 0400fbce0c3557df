"""What the GPU tests of the single stages behind the meters (blend, high-cut, leveller) share: status rows and PCM compared with
their models', and input rows at a chosen address modulo 16."""
import numpy as np


def same_status(got, want, names):
    """the fields `names` of two status arrays, bit for bit; a NaN equals a NaN"""
    for k in names:
        x, y = got[k], want[k]
        if x.dtype.kind == "f":
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            ok = (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert ok.all(), (k, np.flatnonzero(~ok)[:5], x[~ok][:5], y[~ok][:5])


def same_pcm(oracle, got, want, wrap):
    """got [N, n, ac] int16 is the oracle's pack of the model's rows `want` [N, ac, n]"""
    want_pcm = oracle.pcm16(np.ascontiguousarray(np.transpose(want, (0, 2, 1))).reshape(-1), wrap).reshape(got.shape)
    assert np.array_equal(got, want_pcm)


def offset_rows(x, byte_offset):
    """a copy of x whose address is byte_offset modulo 16"""
    pad = np.zeros(x.size + 8, np.float32)
    o = ((byte_offset - pad.ctypes.data) % 16) // 4
    v = pad[o:o + x.size].reshape(x.shape)
    v[...] = x
    assert v.ctypes.data % 16 == byte_offset
    return v
