"""The host transforms Resize and RandomResizedCrop (ringdp.data.transforms): shapes, the bilinear definition, and
boxes that stay inside the image."""
import pytest
import torch
import torch.nn.functional as F

from ringdp.data.transforms import RandomResizedCrop, Resize


@pytest.mark.parametrize("shape", [(28, 28), (32, 32, 3), (7, 9, 3)])
@pytest.mark.parametrize("size", [16, 40])
def test_resize_is_interpolate(shape, size):
    img = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    out = Resize(size)(img)
    assert out.dtype == torch.uint8 and out.shape == (size, size, *shape[2:])
    chw = img.reshape(*shape[:2], -1).permute(2, 0, 1)[None].float()
    want = F.interpolate(chw, (size, size), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    assert torch.equal(out.reshape(size, size, -1), want.round().to(torch.uint8))
    crop = RandomResizedCrop(size, generator=torch.Generator().manual_seed(2))(img)
    assert crop.dtype == torch.uint8 and crop.shape == out.shape


@pytest.mark.parametrize("H,W,ratio", [(32, 32, (3 / 4, 4 / 3)), (7, 9, (3 / 4, 4 / 3)), (8, 40, (0.5, 2.0))])
def test_random_boxes_stay_inside(H, W, ratio):
    t = RandomResizedCrop(16, ratio=ratio, generator=torch.Generator().manual_seed(3))
    areas = set()
    for _ in range(1000):
        y0, x0, h, w = t.get_params(H, W)
        assert 1 <= h <= H and 1 <= w <= W and 0 <= y0 <= H - h and 0 <= x0 <= W - w
        areas.add(h * w)
    assert len(areas) > 5
    with pytest.raises(ValueError):
        RandomResizedCrop(16, scale=(0.9, 0.1))
