"""A/B of the strip A loader against the per-tap loader of the fp32 3x3 convolution, per role, at the bench shapes.

    python scripts/bench_conv_strip.py [frames=1024] [rounds=5]

Alternates default dispatch / GOALNET_F32_CONV_STRIP=0 `rounds` times in one process (the switch is read per call) and
prints median and min-max of both, the median gain and whether it exceeds the min-max spread of the per-tap repeats (the
adoption rule). With GOALNET_LIB_PATH pointing at a library without the strip loader both columns time the same kernel:
that is the check that the switched-off path times like the parent."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cvml_goalnet_amd import _lib, ops

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda:0"
torch.manual_seed(0)


def timeit(fn, reps=3):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def role(name, h, w, cin, cout, affine):
    x = torch.randn(n, h, w, cin, device=dev)
    sc = torch.rand(cin, device=dev) + 0.5 if affine else None
    sh = torch.randn(cin, device=dev) * 0.1 if affine else None
    wt = torch.randn(cout, 3, 3, cin, device=dev) * 0.05
    b = torch.randn(cout, device=dev) if affine else None
    y = torch.empty(n, h, w, cout, device=dev)
    fn = lambda: ops.conv3x3_fwd(x, sc, sh, wt, b, affine, y, n, h, w, cin, cout)
    fl = 2.0 * n * h * w * 9 * cin * cout
    os.environ.pop("GOALNET_F32_CONV_STRIP", None)
    kn = _lib.load().goalnet_conv3x3_fwd_kernel_name(n, h, w, cin, cout, int(affine)).decode()
    loader = kn[kn.index("AL = ") + 5:].split(",")[0].replace("(anonymous namespace)::", "")
    fn(); y_on = y.clone()
    os.environ["GOALNET_F32_CONV_STRIP"] = "0"
    fn(); same = torch.equal(y, y_on)
    del y_on
    on, off = [], []
    for _ in range(rounds):
        os.environ.pop("GOALNET_F32_CONV_STRIP", None)
        on.append(timeit(fn))
        os.environ["GOALNET_F32_CONV_STRIP"] = "0"
        off.append(timeit(fn))
    os.environ.pop("GOALNET_F32_CONV_STRIP", None)
    mon, moff = statistics.median(on), statistics.median(off)
    spread = max(off) - min(off)
    print(f"{name:34s} default [{loader}]: {mon:8.3f} ms ({min(on):.3f}-{max(on):.3f}) {fl / mon / 1e9:6.1f} TF/s | "
          f"STRIP=0: {moff:8.3f} ms ({min(off):.3f}-{max(off):.3f}) {fl / moff / 1e9:6.1f} TF/s | "
          f"gain {moff - mon:+.3f} ms vs per-tap spread {spread:.3f} ms -> {'ADOPT' if moff - mon > spread else 'keep per-tap'}"
          f" | outputs bit-identical: {same}", flush=True)


print(f"N = {n} frames, {rounds} alternations, library {_lib.LIB_PATH}", flush=True)
role("conv3 fwd   72x72 256->512 affine", 72, 72, 256, 512, True)
role("conv3 dgrad 72x72 512->256", 72, 72, 512, 256, False)
role("conv2 fwd   74x74  64->256 affine", 74, 74, 64, 256, True)
role("conv2 dgrad 74x74 256->64 (N64)", 74, 74, 256, 64, False)
