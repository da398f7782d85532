"""What the CPU and GPU mixup tests share: the invariants every mixup record has to satisfy (written from the record
definition in ``ringdp.ops.mixup``, not from the kernel), a two-sample Kolmogorov-Smirnov distance, and the
expectation of a mixed batch built from records with plain torch ops."""
import numpy as np
import torch


def fields(rec):
    """``rec``: int32 array [R, 8] -> dict of per-record arrays (lam, lam0 as float32)."""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int32))
    f = rec.view(np.float32)
    return dict(lam=f[:, 0], kind=rec[:, 1], y0=rec[:, 2], y1=rec[:, 3], x0=rec[:, 4], x1=rec[:, 5], lam0=f[:, 6],
                pad=rec[:, 7])


def box_lam(y0, y1, x0, x1, H, W):
    """lam of a cutmix box, every operation in fp32 as the record definition says."""
    area = np.float32((y1 - y0) * (x1 - x0))
    return np.float32(1.0) - area / np.float32(H * W)


def check_records(rec, H, W):
    """Assert the invariants of the issue's record table; returns the fields."""
    f = fields(rec)
    assert np.all(np.isin(f["kind"], (0, 1, 2))) and np.all(f["pad"] == 0)
    assert np.all((f["lam"] >= 0) & (f["lam"] <= 1)) and np.all((f["lam0"] >= 0) & (f["lam0"] <= 1))
    plain = f["kind"] != 2
    for k in ("y0", "y1", "x0", "x1"):
        assert np.all(f[k][plain] == 0), k  # kinds 0 and 1: the empty box
    assert np.all(f["lam"][f["kind"] == 0] == 1)
    assert np.all(f["lam"][f["kind"] == 1] == f["lam0"][f["kind"] == 1])
    for r in np.nonzero(f["kind"] == 2)[0]:
        y0, y1, x0, x1 = (int(f[k][r]) for k in ("y0", "y1", "x0", "x1"))
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W, (r, y0, y1, x0, x1)
        ratio = np.sqrt(1.0 - float(f["lam0"][r]))
        assert y1 - y0 <= int(H * ratio) + 1 and x1 - x0 <= int(W * ratio) + 1, (r, y0, y1, x0, x1, f["lam0"][r])
        want = box_lam(y0, y1, x0, x1, H, W)
        assert f["lam"][r].tobytes() == want.tobytes(), (r, f["lam"][r], want)
    return f


def ks_distance(a, b):
    """Two-sample Kolmogorov-Smirnov distance: sup |F_a - F_b| over the pooled sample."""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    pooled = np.concatenate([a, b])
    fa = np.searchsorted(a, pooled, side="right") / a.size
    fb = np.searchsorted(b, pooled, side="right") / b.size
    return float(np.abs(fa - fb).max())


def make_record(lam=1.0, kind=0, box=(0, 0, 0, 0), lam0=None):
    """One hand-made record row (int32 [8])."""
    f = np.array([lam, lam if lam0 is None else lam0], dtype=np.float32).view(np.int32)
    return np.array([f[0], kind, *box, f[1], 0], dtype=np.int32)


def expected_mix(x, rec):
    """Expectation of ``mix_images`` for ``x [B, C, H, W]`` (any device / layout) and records int32 [R, 8] (numpy).
    Returns ``(kind [B], copied, blended)``: ``copied`` is what kinds 0 and 2 must equal bit for bit, ``blended`` the
    fp64 value ``lam * a + (1 - lam) * b`` of kind 1, with ``1 - lam`` formed in fp32 as the kernel's contract says.
    The middle sample of an odd batch is its own partner and counts as kind 0."""
    B, _, H, W = x.shape
    f = fields(rec)
    if f["kind"].size == 1:
        f = {k: np.repeat(v, B) for k, v in f.items()}
    kind = f["kind"].copy()
    if B % 2:
        kind[B // 2] = 0
    dev = x.device

    def col(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dtype).view(B, 1, 1, 1)

    hh = torch.arange(H, device=dev).view(1, 1, H, 1)
    ww = torch.arange(W, device=dev).view(1, 1, 1, W)
    box = (hh >= col(f["y0"], torch.int64)) & (hh < col(f["y1"], torch.int64)) \
        & (ww >= col(f["x0"], torch.int64)) & (ww < col(f["x1"], torch.int64))
    other = x.flip(0)
    copied = torch.where(col(kind == 2, torch.bool) & box, other, x)
    rest = (np.float32(1.0) - f["lam"]).astype(np.float32)
    blended = col(f["lam"], torch.float64) * x.double() + col(rest, torch.float64) * other.double()
    return torch.as_tensor(kind, device=dev), copied, blended
