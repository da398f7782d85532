"""The fp8 recipe switch: ``set_fp8`` keeps the per-tensor recipe unless asked for MXFP8."""
import pytest


def test_fp8_recipe_switch(monkeypatch):
    from ringdp.ops.transformer import fp8_enabled, fp8_recipe, set_fp8

    monkeypatch.delenv("RINGDP_FP8_RECIPE", raising=False)
    try:
        set_fp8(True)
        assert fp8_enabled() and fp8_recipe() == "tensor"
        set_fp8(True, recipe="mx")
        assert fp8_enabled() and fp8_recipe() == "mx"
        set_fp8(False)
        assert not fp8_enabled() and fp8_recipe() == "tensor"
        monkeypatch.setenv("RINGDP_FP8_RECIPE", "mx")
        set_fp8(True)
        assert fp8_recipe() == "mx"
        set_fp8(True, recipe="tensor")  # an explicit recipe wins over the environment
        assert fp8_recipe() == "tensor"
        with pytest.raises(ValueError):
            set_fp8(True, recipe="block128")
        assert fp8_enabled() and fp8_recipe() == "tensor"  # a rejected call changes nothing
    finally:
        monkeypatch.delenv("RINGDP_FP8_RECIPE", raising=False)
        set_fp8(False)
    assert not fp8_enabled() and fp8_recipe() == "tensor"
