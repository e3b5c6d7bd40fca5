"""A/B of the buffer-store epilogue of the fp32 GEMM tiles against the per-store-predicated one, per role, at the bench shapes.

    python scripts/bench_epi_store.py [frames=1024] [rounds=5]

Alternates default dispatch / GOALNET_F32_EPI_STORE=0 `rounds` times in one process (the switch is read per call; median of three
launches per turn) and prints median and min-max of both, the median gain and whether it exceeds the min-max spread of the
old-path repeats (the adoption rule). linear5 dX, whose lanes hold adjacent columns, also times GOALNET_F32_EPI_STORE=1, the 4-byte
buffer stores without the 8-byte pairing, in the same alternation: the pairing stays only while it beats that. Outputs of all
settings are compared with torch.equal. With GOALNET_LIB_PATH pointing at a library without the new epilogue every column times
the same kernel: the check that the switched-off path times like the parent."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cvml_goalnet_amd import _lib, ops

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda:0"
ENV = "GOALNET_F32_EPI_STORE"
torch.manual_seed(0)


def setting(s):
    if s is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = s


def timeit(fn, reps=3):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def ab(name, fn, out, fl, pairable):
    settings = [None, "0"] + (["1"] if pairable else [])
    setting("0"); fn(); ref = out.clone()
    same = True
    for s in settings[:1] + settings[2:]:
        setting(s); fn(); same = same and torch.equal(out, ref)
    del ref
    t = {s: [] for s in settings}
    for _ in range(rounds):
        for s in settings:
            setting(s)
            t[s].append(timeit(fn))
    setting(None)
    med = {s: statistics.median(v) for s, v in t.items()}
    spread = max(t["0"]) - min(t["0"])
    gain = med["0"] - med[None]
    line = (f"{name:36s} default: {med[None]:8.3f} ms ({min(t[None]):.3f}-{max(t[None]):.3f}) {fl / med[None] / 1e9:6.1f} TF/s | "
            f"=0: {med['0']:8.3f} ms ({min(t['0']):.3f}-{max(t['0']):.3f}) {fl / med['0'] / 1e9:6.1f} TF/s | "
            f"gain {gain:+.3f} ms ({100 * gain / med['0']:+.2f} %) vs old-path spread {spread:.3f} ms -> "
            f"{'ABOVE the spread' if gain > spread else 'within the spread'}")
    if pairable:
        line += (f" | =1 (no pairing): {med['1']:8.3f} ms ({min(t['1']):.3f}-{max(t['1']):.3f}); pairing {med['1'] - med[None]:+.3f} ms")
    print(line + f" | outputs bit-identical: {same}", flush=True)


def conv(name, h, w, cin, cout, affine):
    x = torch.randn(n, h, w, cin, device=dev)
    sc = torch.rand(cin, device=dev) + 0.5 if affine else None
    sh = torch.randn(cin, device=dev) * 0.1 if affine else None
    wt = torch.randn(cout, 3, 3, cin, device=dev) * 0.05
    b = torch.randn(cout, device=dev) if affine else None
    y = torch.empty(n, h, w, cout, device=dev)
    ab(name, lambda: ops.conv3x3_fwd(x, sc, sh, wt, b, affine, y, n, h, w, cin, cout), y, 2.0 * n * h * w * 9 * cin * cout, False)


def dx5(name, j, k):
    dy = torch.randn(n, j, device=dev)
    wt = torch.randn(j, k, device=dev) * 0.01
    dx = torch.empty(n, k, device=dev)
    ab(name, lambda: ops.linear_bwd_dx(dy, wt, dx), dx, 2.0 * n * j * k, True)


def wgrad(name, h, w, cin, cout):
    x = torch.randn(n, h, w, cin, device=dev)
    dy = torch.randn(n, h, w, cout, device=dev)
    sc = torch.rand(cin, device=dev) + 0.5
    sh = torch.randn(cin, device=dev) * 0.1
    dw = torch.empty(cout, 3, 3, cin, device=dev)
    ab(name, lambda: ops.conv3x3_wgrad(x, sc, sh, dy, dw, n, h, w, cin, cout), dw, 2.0 * n * h * w * 9 * cin * cout, False)


print(f"N = {n} frames, {rounds} alternations, library {_lib.LIB_PATH}", flush=True)
conv("conv3 fwd   72x72 256->512 affine", 72, 72, 256, 512, True)
conv("conv3 dgrad 72x72 512->256", 72, 72, 512, 256, False)
conv("conv2 fwd   74x74  64->256 affine", 74, 74, 64, 256, True)
conv("conv2 dgrad 74x74 256->64 (N64)", 74, 74, 256, 64, False)
dx5("linear5 dX  512 -> 512x70x70", 512, 512 * 70 * 70)
wgrad("conv3 wgrad 72x72 256->512 affine", 72, 72, 256, 512)
