"""CPU: goalnet_conv3x3_fwd_kernel_name mirrors the strip / per-tap dispatch of goalnet_conv3x3_fwd (no launch, no device)."""
import pytest

from cvml_goalnet_amd import _lib

# the roles that take the strip loader (profiles/conv_strip_kernel_stats.md): affine = 1 is the forward, 0 the data gradient
ADOPTED = {"forward": True, "dgrad": True}
STRIP_MAX_W = 79


def name(n, h, w, cin, cout, affine):
    return _lib.load().goalnet_conv3x3_fwd_kernel_name(n, h, w, cin, cout, affine).decode()


def is_strip(s):
    assert "gemm_f32_kernel" in s, s          # bench.py's roofline label hard-codes the base name
    return "ConvAStripLoader" in s


def is_per_tap(s):
    assert "gemm_f32_kernel" in s, s
    return "ConvALoader" in s and "ConvAStripLoader" not in s


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("GOALNET_F32_CONV_STRIP", raising=False)
    monkeypatch.delenv("GOALNET_F32_N64_OFF", raising=False)


def test_bench_shapes_take_the_adopted_loader():
    assert is_strip(name(1024, 72, 72, 256, 512, 1)) == ADOPTED["forward"]
    assert is_strip(name(1024, 74, 74, 64, 256, 1)) == ADOPTED["forward"]
    assert is_strip(name(1024, 72, 72, 512, 256, 0)) == ADOPTED["dgrad"]
    assert is_per_tap(name(1024, 74, 74, 256, 64, 0))       # conv2's data gradient: the 128 x 64 tile keeps the per-tap loader
    for s in (name(1024, 72, 72, 256, 512, 1), name(1024, 72, 72, 512, 256, 0)):
        assert is_strip(s) or is_per_tap(s)


def test_switch_forces_the_per_tap_loader(monkeypatch):
    monkeypatch.setenv("GOALNET_F32_CONV_STRIP", "0")
    assert is_per_tap(name(1024, 72, 72, 256, 512, 1))
    assert is_per_tap(name(1024, 74, 74, 64, 256, 1))
    assert is_per_tap(name(1024, 72, 72, 512, 256, 0))


def test_width_limit():
    assert is_strip(name(1024, 20, STRIP_MAX_W, 32, 512, 1)) == ADOPTED["forward"]
    assert is_per_tap(name(1024, 20, STRIP_MAX_W + 1, 32, 512, 1))
    assert is_per_tap(name(1024, 20, 224, 32, 512, 0))


def test_split_k_keeps_the_per_tap_loader():
    assert _lib.load().goalnet_conv3x3_fwd_ws_bytes(2, 11, 11, 256, 512) > 0
    assert is_per_tap(name(2, 11, 11, 256, 512, 1))
    assert is_per_tap(name(2, 11, 11, 512, 256, 0))
