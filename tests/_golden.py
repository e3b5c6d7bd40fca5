"""Reader/checker for the tests/golden/*.npz fixtures (written FROM THE REFERENCE by make_golden.py).

A fixture holds, per named tensor, either the whole tensor (<= 4096 elements) or {sum, sum of squares,
abs-max} plus 64 sampled elements. Sample indices derive from the tensor's base name, so a parameter's
gradient (`sK.grad.X`) and its updated value (`sK.param.X`) are sampled at the same places."""
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
NSAMPLES = 64


def _salt(key: str) -> int:
    base = key.split(".", 2)[2] if key[0] == "s" and key[1].isdigit() else key
    return zlib.crc32(base.encode()) & 0xFFFF


class Golden:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.n = int(self.z["meta|n"][0]); self.h = int(self.z["meta|h"][0])
        self.steps = int(self.z["meta|steps"][0]); self.audio = bool(self.z["meta|audio"][0])
        self.drop = bool(self.z["meta|drop"][0])
        self.bins = int(self.z["meta|bins"][0]) if "meta|bins" in self.z.files else 30      # audio bin length; stored where it is not 30

    def keys(self, prefix):
        return sorted({k.split("|")[0] for k in self.z.files if k.startswith(prefix)})

    def numel(self, key):
        return int(np.prod(self.z[key + "|shape"])) if len(self.z[key + "|shape"]) else 1

    def samples(self, key):
        """(flat indices, reference values as float64) — all elements for small tensors."""
        from cvml_goalnet_amd import synth
        if key + "|full" in self.z.files:
            g = self.z[key + "|full"].astype(np.float64)
            return np.arange(g.size), g
        idx = synth.sample_indices(self.numel(key), NSAMPLES, _salt(key))
        return idx, self.z[key + "|samples"].astype(np.float64)

    def absmax(self, key):
        if key + "|full" in self.z.files:
            g = self.z[key + "|full"]
            return float(np.abs(g).max()) if g.size else 0.0
        return float(self.z[key + "|stats"][2])

    def flat(self, t):
        import torch
        return t.detach().to("cpu", torch.float64).reshape(-1).numpy()

    def check(self, key, t, rtol, atol=0.0, what="", stats_rtol=None):
        """Compare tensor `t` (torch; logical torch-native shape) with the stored summary: sampled (or all)
        elements within atol + rtol * max|ref|; for large tensors also the sum of squares and the abs-max.
        Returns max error / max|ref|."""
        a = self.flat(t)
        assert self.numel(key) == a.size, f"{key}: numel {a.size} vs golden shape {tuple(self.z[key + '|shape'])}"
        idx, g = self.samples(key)
        scale = max(self.absmax(key), 1e-30)
        err = float(np.abs(a[idx] - g).max()) if g.size else 0.0
        assert err <= atol + rtol * scale, f"{self.name}:{key}{what}: max abs err {err:.3e} (scale {scale:.3e}, tol {atol + rtol * scale:.3e})"
        if key + "|stats" in self.z.files:
            stats = self.z[key + "|stats"]
            sr = stats_rtol if stats_rtol is not None else max(4 * rtol, 1e-6)
            ss = float((a * a).sum())
            assert abs(ss - stats[1]) <= sr * max(stats[1], 1e-30) + atol * atol * a.size, \
                f"{self.name}:{key}{what}: sum of squares {ss} vs {stats[1]}"
            amax = float(np.abs(a).max())
            assert abs(amax - stats[2]) <= max(rtol, 1e-6) * scale + atol, f"{self.name}:{key}{what}: absmax {amax} vs {stats[2]}"
        return err / scale


GOLDEN_CASES_SMALL = ["avm_a1_n10_h40_p0", "avm_a1_n10_h40_mask3", "avm_a0_n10_h40_mask", "avm_a1_n1_h40_p0",
                      "avm_a1_n16_h40_mask", "avm_a0_n7_h52_p0", "avm_a1_n10_h40_b60_p0", "avm_a1_n7_h40_b17_mask"]
GOLDEN_CASES_BIG = ["avm_a1_n2_h224_p0"]


POSTPROC_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("postproc_") and f.endswith(".npz"))


def load_postproc(name):
    """tests/golden/postproc_*.npz (written by make_golden_postproc.py from the reference's own functions): inputs
    pred (N,1), change_points (n_clips,2), gd (20,N_raw), skip, full_n; outputs importances, expanded, clip_values,
    clip_lengths, capacity, selected, mask, fscore."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}
