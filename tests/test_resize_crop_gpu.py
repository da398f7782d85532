"""Random-resized-crop + bilinear resize on the GPU (csrc/kernels/resize_crop.hip): the image kernel against an fp64
oracle built with F.interpolate from hand-made records, the drawn records (invariants, law, determinism), the
DeviceLoader wiring, a captured batch that re-augments on every replay, and the errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixup_common as mc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SNAPS = [(1234, 1), (2 ** 63 + 2 ** 40 + 7, 2 ** 32 + 5)]  # the second: high bits set in the seed and in the step
MEAN, STD = (0.4, 0.5, 0.45), (0.25, 0.3, 0.35)
ERR = (RuntimeError, ValueError, TypeError)


def _snap(seed, step):
    s = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed, step)]
    return torch.tensor(s, dtype=torch.int64, device=DEV)


def _rec(box, flip=0, erows=(0, 0), ecols=(0, 0)):
    return [*box, flip, erows[0] | erows[1] << 16, ecols[0] | ecols[1] << 16, 0]


def oracle(x, idx, rec, S, mean, std):
    """fp64 expectation [B, C, S, S] and the erase mask, straight from the definition.  ``x`` uint8 [N, H, W(, C)]."""
    x = x.cpu() if x.dim() == 4 else x.cpu().unsqueeze(-1)
    C = x.shape[3]
    rec = np.broadcast_to(np.asarray(rec), (len(idx), 8))
    m = torch.tensor(mean[:C], dtype=torch.float64).view(C, 1, 1)
    s = torch.tensor(std[:C], dtype=torch.float64).view(C, 1, 1)
    outs, masks = [], []
    for b, i in enumerate(idx):
        y0, x0, h, w, flip, er, ec, _ = (int(v) for v in rec[b])
        crop = x[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].double()
        o = F.interpolate(crop, (S, S), mode="bilinear", align_corners=False)[0]
        o = ((o.flip(2) if flip else o) / 255.0 - m) / s
        mask = torch.zeros(S, S, dtype=torch.bool)
        mask[er & 0xffff:er >> 16, ec & 0xffff:ec >> 16] = True
        outs.append(o.masked_fill(mask, 0.0))
        masks.append(mask.expand(C, S, S))
    return torch.stack(outs), torch.stack(masks)


def check_images(out, ref, mask, src_hw, std, C):
    """The issue's tolerance: fp32 coordinate error times one grey level of slope, plus half a bf16 ulp for bf16."""
    atol = 64 * 2.0 ** -23 * max(src_hw) / min(std[:C])
    rtol = 2.0 ** -8 if out.dtype == torch.bfloat16 else 0.0
    got = out.cpu().double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    print(f"max err {float(err.max()):.3e}  atol {atol:.3e}  rtol {rtol:.3e}")
    assert bool((err <= atol + rtol * ref.abs()).all()), float((err - rtol * ref.abs()).max())
    assert bool((got[mask] == 0).all())


# ------------------------------------------------------------------------------------------------ 1. images
@pytest.mark.parametrize("shape,S", [((32, 32, 3), 224), ((28, 28), 36), ((32, 32, 3), 16)],
                         ids=["up224", "grey36", "down16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_images_from_records(dtype, channels_last, shape, S):
    from ringdp.ops.resize_crop import resize_crop

    H, W = shape[:2]
    C = shape[2] if len(shape) == 3 else 1
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (9, *shape), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (9,), generator=g)
    idx = [7, 2, 7, 0, 5]
    recs = np.array([
        _rec((0, 0, H, W)),                                          # the whole image, empty erase box
        _rec((3, 4, 1, 1), erows=(0, S), ecols=(0, S)),              # 1 x 1 box; everything erased
        _rec((H - 10, W - 7, 10, 7), erows=(2, 5), ecols=(9, 14)),   # bottom-right corner; erase inside one 8-vector
        _rec((0, 5, H, 1), flip=1),                                  # one pixel wide, full height, flipped
        _rec((2, 3, H - 5, W - 9), flip=1, erows=(1, S - 1), ecols=(3, S - 2)),  # erase edges inside vectors
    ], dtype=np.int32)
    xd, yd, idxd = x.to(DEV), y.to(DEV), torch.tensor(idx, device=DEV)
    for rec in (recs, recs[4:5]):  # a record per sample, then one [1, 8] record for the batch
        out, yo = resize_crop(xd, yd, idxd, torch.from_numpy(rec).to(DEV), S, MEAN[:C], STD[:C], channels_last, dtype)
        assert out.dtype == dtype and out.shape == (5, C, S, S)
        assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        assert torch.equal(yo.cpu(), y[idx])
        ref, mask = oracle(x, idx, rec, S, MEAN, STD)
        check_images(out, ref, mask, (H, W), STD, C)


# ------------------------------------------------------------------------------------------------ 2. records
def _fields(rec):
    r = rec.cpu().numpy().astype(np.int64)
    return dict(y0=r[:, 0], x0=r[:, 1], h=r[:, 2], w=r[:, 3], flip=r[:, 4], ey0=r[:, 5] & 0xffff, ey1=r[:, 5] >> 16,
                ex0=r[:, 6] & 0xffff, ex1=r[:, 6] >> 16, pad=r[:, 7])


def _check_records(rec, H, W, S):
    f = _fields(rec)
    assert np.all((f["h"] >= 1) & (f["w"] >= 1) & (f["y0"] >= 0) & (f["x0"] >= 0))
    assert np.all((f["y0"] + f["h"] <= H) & (f["x0"] + f["w"] <= W))
    assert np.all(np.isin(f["flip"], (0, 1))) and np.all(f["pad"] == 0)
    eh, ew = f["ey1"] - f["ey0"], f["ex1"] - f["ex0"]
    empty = (eh == 0) & (ew == 0)
    assert np.all(empty | ((eh >= 1) & (ew >= 1) & (eh < S) & (ew < S) & (f["ey1"] <= S) & (f["ex1"] <= S)))
    return f, ~empty


def _simulate_area(n, H, W, scale, ratio, rng):
    """torchvision's RandomResizedCrop.get_params in numpy: the area fraction h * w / (H * W) of n draws."""
    h, w, done = np.full(n, H), np.full(n, W), np.zeros(n, dtype=bool)
    if W / H < ratio[0]:
        h[:] = int(round(W / ratio[0]))
    elif W / H > ratio[1]:
        w[:] = int(round(H * ratio[1]))
    for _ in range(10):
        area = H * W * rng.uniform(scale[0], scale[1], n)
        ar = np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1]), n))
        cw, ch = np.rint(np.sqrt(area * ar)), np.rint(np.sqrt(area / ar))
        ok = ~done & (cw >= 1) & (cw <= W) & (ch >= 1) & (ch <= H)
        h[ok], w[ok] = ch[ok], cw[ok]
        done |= ok
    return h * w / (H * W)


@pytest.mark.parametrize("seed,step", SNAPS, ids=["low", "high"])
@pytest.mark.parametrize("H,W,S", [(32, 32, 224), (28, 28, 36), (7, 9, 16)])
def test_drawn_records(H, W, S, seed, step):
    from ringdp.ops.resize_crop import crop_records

    R = 16384
    kw = dict(hflip=True, erase_prob=0.25)
    rec = crop_records(_snap(seed, step), R, H, W, S, **kw)
    assert rec.shape == (R, 8) and rec.dtype == torch.int32
    f, erased = _check_records(rec, H, W, S)
    assert torch.equal(rec, crop_records(_snap(seed, step), R, H, W, S, **kw))
    assert not torch.equal(rec, crop_records(_snap(seed, step + 1), R, H, W, S, **kw))
    assert not torch.equal(rec, crop_records(_snap(seed + 1, step), R, H, W, S, **kw))
    off, _ = _check_records(crop_records(_snap(seed, step), R, H, W, S, scale=None), H, W, S)
    assert np.all((off["y0"] == 0) & (off["x0"] == 0) & (off["h"] == H) & (off["w"] == W))
    assert np.all(off["flip"] == 0) and np.all(off["ey1"] == 0) and np.all(off["ex1"] == 0)
    if (H, W) == (32, 32):  # the law, at the default scale and ratio
        want = _simulate_area(R, H, W, (0.08, 1.0), (3 / 4, 4 / 3), np.random.default_rng(5))
        d = mc.ks_distance(f["h"] * f["w"] / (H * W), want)
        print(f"KS distance {d:.4f}  flips {f['flip'].mean():.4f}  erased {erased.mean():.4f}")
        assert d <= 0.03
        assert abs(f["flip"].mean() - 0.5) <= 5 * 0.5 / np.sqrt(R)
        # an erase attempt can draw a box without rows or columns; at S = 224 the smallest area is 1000 pixels
        assert abs(erased.mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / R)


# ------------------------------------------------------------------------------------------------ 3. the loader
def _loader(**kw):
    from ringdp.data import DeviceLoader, SyntheticImages

    ds = SyntheticImages(64, (32, 32, 3), 10, seed=3)
    return ds, DeviceLoader(ds, 8, "cuda", mean=MEAN, std=STD, out_dtype=torch.bfloat16, **kw)


def test_loader_end_to_end():
    import ringdp.random as rr
    from ringdp._native import C

    ds, loader = _loader(resize=40, hflip=True, erase_prob=0.5)

    def two_epochs():
        rr.manual_seed(21, DEV)
        return [b for _ in range(2) for b in loader]

    first, again = two_epochs(), two_epochs()
    assert len(first) == 16 and rr.get_rng_state(DEV) == (21, 16)
    for k, ((xa, ya), (xb, yb)) in enumerate(zip(first, again)):
        assert xa.shape == (8, 3, 40, 40) and xa.dtype == torch.bfloat16
        assert torch.equal(ya.cpu(), ds.targets[8 * (k % 8):8 * (k % 8) + 8])
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(first[0][0], first[8][0])  # the second epoch draws anew
    loader.eval()
    xe, ye = next(iter(loader))
    assert rr.get_rng_state(DEV) == (21, 16)  # nothing drawn
    ref, mask = oracle(ds.data, range(8), _rec((0, 0, 32, 32)), 40, MEAN, STD)
    check_images(xe, ref, mask, (32, 32), STD, 3)
    _, plain = _loader(hflip=True, crop_padding=2)  # resize=None: the launch it always was
    idx = torch.arange(5, 13, device=DEV)
    xp, yp = plain.batch(idx, 77)
    xg, yg = C.gather_augment(plain.x, plain.y, idx, 2, True, list(MEAN), list(STD), 77, False, torch.bfloat16)
    assert torch.equal(xp, xg) and torch.equal(yp, yg)


# ------------------------------------------------------------------------------------------------ 4. capture
def test_captured_batch_reaugments():
    import ringdp.random as rr

    _, loader = _loader(resize=40, hflip=True, erase_prob=0.5)
    idx = torch.arange(8, device=DEV)
    rr.manual_seed(9, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loader.batch(idx, 0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, _ = loader.batch(idx, 0)
    torch.cuda.synchronize()
    state = rr.get_rng_state(DEV)
    first = []
    for _ in range(3):
        graph.replay()
        first.append(out.clone())
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    rr.set_rng_state(state, DEV)
    for want in first:
        graph.replay()
        assert torch.equal(out, want)
    rr.set_rng_state(state, DEV)
    for want in first:  # and the eager batches of the same states
        assert torch.equal(loader.batch(idx, 0)[0], want)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors():
    import ringdp.random as rr
    from ringdp._native import C
    from ringdp.data import DeviceLoader, SyntheticImages
    from ringdp.ops.resize_crop import crop_records, resize_crop

    rr.manual_seed(4, DEV)
    x = torch.zeros(4, 32, 32, 3, dtype=torch.uint8, device=DEV)
    idx = torch.arange(2, device=DEV)
    rec = torch.tensor([_rec((0, 0, 32, 32))] * 2, dtype=torch.int32, device=DEV)
    snap = _snap(1, 1)
    resize_crop(x, None, idx, rec, 8)  # the arguments the bad calls vary are good
    bad_calls = [
        lambda: resize_crop(torch.zeros(2, 128, 128, 3, dtype=torch.uint8, device=DEV), None, idx, rec, 8),  # 48 KiB
        lambda: resize_crop(x, None, idx, rec, 0),
        lambda: resize_crop(x, None, idx, rec[:, :7].contiguous(), 8),
        lambda: resize_crop(x, None, idx, torch.cat([rec, rec, rec]), 8),
        lambda: resize_crop(x, None, idx, rec.long(), 8),
        lambda: resize_crop(x.cpu(), None, idx, rec, 8),
        lambda: resize_crop(x, None, idx.cpu(), rec, 8),
        lambda: resize_crop(x, None, idx, rec.cpu(), 8),
        lambda: resize_crop(x, None, idx, rec, 8, out_dtype=torch.float16),
        lambda: crop_records(snap.cpu(), 4, 32, 32, 8),
        lambda: crop_records(snap, 4, 32, 32, 0),
        lambda: crop_records(snap, 4, 32, 32, 8, scale=(0.9, 0.1)),
        lambda: crop_records(snap, 4, 32, 32, 8, ratio=(2.0, 0.5)),
        lambda: C.crop_draw(snap, 4, 32, 32, 8, (0.9, 0.1), (0.75, 1.33), False, 0.0, (0.02, 0.33), (0.3, 3.3)),
        lambda: C.crop_draw(snap, 4, 32, 32, 8, (0.1, 0.9), (2.0, 0.5), False, 0.0, (0.02, 0.33), (0.3, 3.3)),
    ]
    ds = SyntheticImages(8, (32, 32, 3))
    for kw in (dict(crop_padding=4), dict(crop_scale=(0.9, 0.1)), dict(crop_ratio=(2.0, 0.5)), dict(resize=0),
               dict(out_dtype=torch.uint8)):
        bad_calls.append(lambda kw=kw: DeviceLoader(ds, 4, "cuda", **{"resize": 16, **kw}))
    bad_calls.append(lambda: DeviceLoader(SyntheticImages(2, (128, 128, 3)), 2, "cuda", resize=16))
    for k, call in enumerate(bad_calls):
        with pytest.raises(ERR):
            call()
            pytest.fail(f"bad call {k} did not raise")
    assert rr.get_rng_state(DEV) == (4, 0)
