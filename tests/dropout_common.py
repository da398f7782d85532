"""numpy oracle of ringdp's dropout masks (``ringdp.ops.dropout``: Philox4x32-10, counter = (group, step lo, step hi,
site), key = seed) and the mask builders the CPU and GPU tests share.  Written from the mask definition, not from
the kernel: the GPU has to match it bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (uint arrays or ints); returns four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _U32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & _U32, int(k1) & _U32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_U32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_U32)]
        k0, k1 = (k0 + W0) & _U32, (k1 + W1) & _U32
    return [w.astype(np.uint32) for w in c]


def quantize(p):
    """(thr, scale as np.float32) - the definition, independent of ringdp.ops.dropout.quantize_p."""
    thr = min(max(int(round(p * 65536.0)), 0), 65535)
    return thr, np.float32(65536.0 / (65536 - thr))


def _words(groups, seed, step, site):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10(groups, step & _U32, step >> 32, site, seed & _U32, seed >> 32)


def element_u16(numel, seed, step, site):
    """The 16-bit draw of every element of a flat tensor of ``numel`` (a multiple of 8) elements."""
    assert numel % 8 == 0
    w = np.stack(_words(np.arange(numel // 8, dtype=np.uint64), seed, step, site), axis=1)  # [groups, 4]
    halves = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=2)                   # [groups, 4, 2]
    return halves.reshape(-1)  # element j of a group: word j >> 1, half j & 1


def element_keep(numel, thr, seed, step, site):
    return element_u16(numel, seed, step, site) >= thr


def row_keep(B, thr, seed, step, site):
    """Keep decision per sample (stochastic depth)."""
    return (_words(np.arange(B, dtype=np.uint64), seed, step, site)[0] & np.uint32(0xFFFF)) >= thr
