"""GPU: the strip A loader of the fp32 3x3 convolution (ConvAStripLoader, csrc/gemm_f32.hip) against the per-tap loader it
replaces and against fp64.

The strip loader stages each 32-channel chunk of a 128-pixel tile once and reads the nine taps as shifted windows of that
one LDS image; the K order and the MFMA sequence per output are those of the per-tap loader, so the two must agree bit for
bit (torch.equal). GOALNET_F32_CONV_STRIP=0, read per call, selects the per-tap loader. Every shape has M-tiles x N-tiles
>= 256, where the forward takes no split-K and the strip loader is eligible.

Accuracy: the bound of tests/test_gpu_ops.py::test_conv3x3_fwd, 5e-6 of max |y| against F.conv2d in fp64 (affine in fp64,
zero padding of the affine's output); on the whole tensor where marked `full`, else on 64 seeded output pixels that
include the four corners of the first and of the last frame.

The W-limit case: at the issue's (2, 20, W, 32 -> 512) the forward has 100 output tiles and takes split-K at any W the
strip can hold, so the strip could never be selected there; six frames (300 tiles) keep the same H, W and channels."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cvml_goalnet_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
RT = 5e-6
STRIP_MAX_W = 79        # 128 + 2 (W + 1) strip rows <= 288 (nine 32-row loads per thread)


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def close(name, got, want, rtol=RT):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    print(f"[parity] {name}: max|err| = {err:.3e}  scale = {scale:.3e}  rel = {err / scale:.3e}")
    assert err <= rtol * scale, f"{name}: err {err:.3e} > {rtol:.1e} * {scale:.3e}"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def kernel_name(n, h, w, cin, cout, affine):
    return _lib.load().goalnet_conv3x3_fwd_kernel_name(n, h, w, cin, cout, int(affine)).decode()


def make_inputs(n, h, w, cin, cout, affine, bias):
    x = rnd(n, h, w, cin, seed=7)
    sc = rnd(cin, seed=8, lo=0.5, hi=1.5) if affine else None
    sh = rnd(cin, seed=9, lo=-0.5, hi=0.5) if affine else None
    wt = rnd(cout, 3, 3, cin, seed=10, lo=-0.05, hi=0.05)
    b = rnd(cout, seed=11) if bias else None
    return x, sc, sh, wt, b


def run(x, sc, sh, wt, b, relu):
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    y = torch.full((n, h, w, cout), float("nan"), device=DEV)
    ops.conv3x3_fwd(x.to(DEV), None if sc is None else sc.to(DEV), None if sh is None else sh.to(DEV), wt.to(DEV),
                    None if b is None else b.to(DEV), relu, y, n, h, w, cin, cout)
    return y.cpu()


def run_both(monkeypatch, x, sc, sh, wt, b, relu, want_strip=True):
    """-> (default path, per-tap path); asserts which loader the default path selected"""
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    monkeypatch.delenv("GOALNET_F32_CONV_STRIP", raising=False)
    name = kernel_name(n, h, w, cin, cout, sc is not None)
    assert "gemm_f32_kernel" in name
    assert ("ConvAStripLoader" in name) == want_strip, name
    y = run(x, sc, sh, wt, b, relu)
    monkeypatch.setenv("GOALNET_F32_CONV_STRIP", "0")
    off = kernel_name(n, h, w, cin, cout, sc is not None)
    assert "ConvALoader" in off and "Strip" not in off, off
    y0 = run(x, sc, sh, wt, b, relu)
    monkeypatch.delenv("GOALNET_F32_CONV_STRIP", raising=False)
    return y, y0


def affine64(x, sc, sh):
    return x.double() * sc.double() + sh.double() if sc is not None else x.double()


def ref_full(x, sc, sh, wt, b, relu):
    ref = F.conv2d(nchw(affine64(x, sc, sh)), wt.double().permute(0, 3, 1, 2), None if b is None else b.double(), padding=1)
    return nhwc(F.relu(ref) if relu else ref)


def sample_pixels(n, h, w, seed=12, count=64):
    """flat pixel indices: the four corners of the first and of the last frame, the rest seeded"""
    corners = [f * h * w + r * w + c for f in (0, n - 1) for r in (0, h - 1) for c in (0, w - 1)]
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, n * h * w, (count,), generator=g).tolist()
    return torch.tensor(list(dict.fromkeys(corners + rest))[:count])


def ref_pixels(x, sc, sh, wt, b, relu, pix):
    """fp64 outputs [len(pix), cout] of the flat pixels `pix`"""
    n, h, w, cin = x.shape
    xp = F.pad(affine64(x, sc, sh), (0, 0, 1, 1, 1, 1))             # zero padding of the affine's OUTPUT
    f, r, c = pix // (h * w), (pix // w) % h, pix % w
    patch = torch.stack([xp[f, r + kh, c + kw] for kh in range(3) for kw in range(3)], dim=1)      # [P, 9, cin]
    ref = patch.reshape(len(pix), -1) @ wt.double().reshape(wt.shape[0], -1).t()
    if b is not None:
        ref = ref + b.double()
    return F.relu(ref) if relu else ref


CASES = [
    # n, h, w, cin, cout, affine, bias, relu, full
    (1000, 3, 3, 64, 512, True, True, True, True),      # every pixel a border pixel, every strip spans ~15 frames
    (300, 30, 1, 32, 512, True, False, False, False),   # W = 1: the kw = 0 and kw = 2 taps are always padding
    (300, 1, 30, 32, 512, True, False, False, False),   # its transpose: the kh = 0 and kh = 2 taps
    (4, 45, 45, 64, 512, True, False, False, True),     # 8100 pixels: ragged last tile (36 rows); two chunks: the strip reload
    (2, 74, 74, 64, 512, True, True, True, False),      # conv2's width; first strip starts in front of the tensor, last ends behind it
    (2, 72, 72, 32, 512, False, False, False, False),   # conv3's width; one chunk, M a multiple of 128
    (4, 72, 72, 96, 256, False, False, False, False),   # the data-gradient form; an odd number of chunks
]


@pytest.mark.parametrize("n,h,w,cin,cout,affine,bias,relu,full", CASES)
def test_strip_equals_per_tap_and_fp64(monkeypatch, n, h, w, cin, cout, affine, bias, relu, full):
    x, sc, sh, wt, b = make_inputs(n, h, w, cin, cout, affine, bias)
    y, y0 = run_both(monkeypatch, x, sc, sh, wt, b, relu)
    assert torch.equal(y, y0), f"strip != per-tap at {(y != y0).sum().item()} of {y.numel()} outputs"
    tag = f"conv_strip[{n}x{h}x{w}x{cin}->{cout}]"
    if full:
        close(tag, y, ref_full(x, sc, sh, wt, b, relu))
    else:
        pix = sample_pixels(n, h, w)
        close(tag + f" {len(pix)} pixels", y.reshape(-1, cout)[pix], ref_pixels(x, sc, sh, wt, b, relu, pix))


@pytest.mark.parametrize("w,strip", [(STRIP_MAX_W, True), (STRIP_MAX_W + 1, False)])
def test_width_limit(monkeypatch, w, strip):
    """the widest W the dispatcher gives to the strip, and W + 1, which must take the per-tap loader and still be right"""
    n, h, cin, cout = 6, 20, 32, 512
    x, sc, sh, wt, b = make_inputs(n, h, w, cin, cout, True, False)
    y, y0 = run_both(monkeypatch, x, sc, sh, wt, b, False, want_strip=strip)
    assert torch.equal(y, y0)
    pix = sample_pixels(n, h, w)
    close(f"conv_strip[W={w}]", y.reshape(-1, cout)[pix], ref_pixels(x, sc, sh, wt, b, False, pix))


def test_nan_in_padding_neighbours(monkeypatch):
    """NaN in pixels that other frames only ever see as padding: the last row of frame 1 and the first row of frame 4.
    The first row of frame 2 and the last row of frame 3 address those pixels with their kh = 0 / kh = 2 taps, which are
    padding: they must read zeros, not the strip's NaN (an address select, no 0 * NaN). Outputs that reach a NaN pixel
    through a valid tap (the last two rows of frame 1, the first two of frame 4) are not finite by definition and left out of
    the fp64 comparison; everything else is held to it, and the two loaders must agree everywhere, NaN positions included.
    (A full convolution sums over all input channels, so the planting cannot be limited to channels without outputs:
    the two plantings sit on different frame pairs instead, which leaves their padding neighbours clean.)"""
    n, h, w, cin, cout = 6, 40, 40, 64, 512           # 9600 pixels: 75 x 4 tiles; two chunks
    x, sc, sh, wt, b = make_inputs(n, h, w, cin, cout, True, True)
    x[1, h - 1] = float("nan")
    x[4, 0] = float("nan")
    y, y0 = run_both(monkeypatch, x, sc, sh, wt, b, False)       # no ReLU: fmaxf(NaN, 0) is 0
    dirty = torch.zeros(n, h, w, dtype=torch.bool)
    dirty[1, h - 2:] = True
    dirty[4, :2] = True
    # the epilogue's fmaxf(v + bias, -inf) turns a NaN accumulator into -inf: "not finite" marks the reached outputs
    assert torch.equal((~torch.isfinite(y)).any(dim=-1), dirty), "NaN leaked through a padding tap (or a valid tap lost it)"
    assert torch.equal((~torch.isfinite(y)).all(dim=-1), dirty)
    assert torch.equal(torch.isnan(y), torch.isnan(y0))
    assert torch.equal(torch.nan_to_num(y), torch.nan_to_num(y0))
    ref = ref_full(torch.nan_to_num(x), sc, sh, wt, b, False)
    clean = ~dirty
    assert clean[2, 0].all() and clean[3, h - 1].all() and clean[0, h - 1].all() and clean[5, 0].all()
    close("conv_strip[NaN planted] clean pixels", y[clean], ref[clean])
