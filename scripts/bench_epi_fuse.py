"""A/B of the fp32 GEMM epilogue fusion against the launches it replaces, per role, at the bench shapes (224 x 224 frames).

    python scripts/bench_epi_fuse.py [frames=1024] [rounds=5] [role ...]

Roles:
  dw_adam   linear5's weight gradient with Adam in its epilogue (ops.linear_bwd_dw_adam) against ops.linear_bwd_dw into a gradient
            buffer followed by ops.adam_step_dev over it

Each role runs in a child process of its own under a time limit; the parent never touches the GPU and stops at the first child
that fails. In the child, fused and unfused alternate `rounds` times in one process, each turn the median of three launches;
printed are median and min-max of both, the median gain and whether it exceeds the min-max spread of the unfused repeats (the
adoption rule of profiles/conv_strip_kernel_stats.md). Before timing, both forms run once from the same state and the results are
compared bit for bit at this size."""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROLES = ("dw_adam",)
CHILD_TIMEOUT_S = 420


def timeit(torch, fn, reps=3):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def report(name, fused, unfused, same, note=""):
    mf, mu = statistics.median(fused), statistics.median(unfused)
    spread = max(unfused) - min(unfused)
    print(f"{name:28s} fused: {mf:8.3f} ms ({min(fused):.3f}-{max(fused):.3f}) | unfused: {mu:8.3f} ms ({min(unfused):.3f}-{max(unfused):.3f}) | "
          f"gain {mu - mf:+.3f} ms vs unfused spread {spread:.3f} ms -> {'ADOPT' if mu - mf > spread else 'keep the launches'}"
          f" | results bit-identical: {same}{note}", flush=True)


def dw_adam(n, rounds):
    import torch
    from cvml_goalnet_amd import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    J, C, HW = 512, 512, 70 * 70
    K = C * HW
    dz5 = torch.randn(n, J, device=dev) * 1e-3
    p3 = torch.randn(n, K, device=dev)
    sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    p = torch.randn(J * K, device=dev) * 0.01
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)

    def fused():
        ops.linear_bwd_dw_adam(dz5, p3, p, m, v, *hyper, step, scale=sc, shift=sh, bnC=C, step_bias=1)

    def unfused():
        ops.linear_bwd_dw(dz5, p3, g, scale=sc, shift=sh, bnC=C)
        ops.adam_step_dev(p, g, m, v, *hyper, step, step_bias=1)

    def gemm_only():
        ops.linear_bwd_dw(dz5, p3, g, scale=sc, shift=sh, bnC=C)

    # one step of each form from the same state, compared bit for bit (the second set of arrays is freed before timing)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    unfused()
    ops.linear_bwd_dw_adam(dz5, p3, p2, m2, v2, *hyper, step, scale=sc, shift=sh, bnC=C, step_bias=1)
    torch.cuda.synchronize()
    same = torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)
    del p2, m2, v2
    f, u = [], []
    for _ in range(rounds):
        f.append(timeit(torch, fused))
        u.append(timeit(torch, unfused))
    gemm = timeit(torch, gemm_only)
    report(f"linear5 dW + Adam, {n} frames", f, u, same, f" | dW alone {gemm:.3f} ms")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        globals()[args[1]](int(args[2]), int(args[3]))
        return
    n = int(args[0]) if len(args) > 0 else 1024
    rounds = int(args[1]) if len(args) > 1 else 5
    roles = args[2:] or ROLES
    print(f"N = {n} frames, {rounds} alternations", flush=True)
    for r in roles:
        if r not in ROLES:
            sys.exit(f"unknown role {r!r}: one of {ROLES}")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", r, str(n), str(rounds)], timeout=CHILD_TIMEOUT_S).returncode
        if rc != 0:
            sys.exit(f"role {r}: child exited with {rc}; nothing more is started")


if __name__ == "__main__":
    main()
