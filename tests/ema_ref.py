"""numpy float64 restatement of the weight average of include/goalnet_ema.h, written from its definition and not
from the kernel. With t the 1-based count of applied optimizer steps:

    t <= start_step                  e = p                                   (the average tracks the weights)
    u = t - start_step, u % every    nothing is written
    otherwise                        k = u / every - 1, d = min(decay, (1 + k) / (10 + k)) under warm-up, else decay
                                     e = e + (1 - d) (p - e)

`weight(t, ...)` -> None (no write) | 1.0 (copy) | 1 - d. `update(e, p, t, ...)` -> the new average, everything in float64 (the copy
included: an fp32 p is exact there). `bound_term(e_before, p)` -> what one averaging write adds to the per-element error bound of the
fp32 kernel against this restatement started from the same fp32 p sequence:

    4 * 2^-24 * max(|p|, |e|)

one rounding each for the difference p - e, the product-sum and the fp32 weight w. With M = max(|p|, |e|) and |p - e| <= 2 M: the
rounded difference is off by at most 2^-24 |p - e| and enters times w (<= 2 w 2^-24 M), the rounded weight is off by at most
2^-24 w and enters times |p - e| (<= 2 w 2^-24 M), the fused multiply-add rounds a result that lies between p and e (<= 2^-24 M):
(4 w + 1) 2^-24 M, inside 4 * 2^-24 M for every w <= 3/4 — the regime of an average, where torch.lerp uses this form — and for the
larger weights the tests run (w = 1: the weight is exact, 3; w = 0.9: fp32(0.9) is off by 0.44 * 2^-24 relative, 3.6). The error
carried over from earlier writes is multiplied by d < 1 and so stays inside the terms already summed. A copy resets the bound to 0:
the kernel's copy is exact."""
import numpy as np

EPS24 = 2.0 ** -24


def weight(t, decay, every=1, start_step=0, warmup=False):
    if t <= start_step:
        return 1.0
    u = t - start_step
    if u % every:
        return None
    k = u // every - 1
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + k) / (10.0 + k))
    return 1.0 - d


def update(e, p, t, decay, every=1, start_step=0, warmup=False):
    """e, p: float64 arrays; returns (new e, wrote: bool, copied: bool)"""
    w = weight(t, decay, every, start_step, warmup)
    p = np.asarray(p, dtype=np.float64)
    if w is None:
        return e, False, False
    if t <= start_step:
        return p.copy(), True, True
    e = np.asarray(e, dtype=np.float64)
    return e + w * (p - e), True, False


def bound_term(e_before, p):
    return 4.0 * EPS24 * np.maximum(np.abs(np.asarray(p, dtype=np.float64)), np.abs(np.asarray(e_before, dtype=np.float64)))


class Tracker:
    """the restatement run beside a device run: feed it every step's post-update fp32 weights; `e` is the fp64 average, `bound` the
    accumulated per-element bound"""

    def __init__(self, e0, decay, every=1, start_step=0, warmup=False):
        self.e = np.asarray(e0, dtype=np.float64).copy()
        self.bound = np.zeros_like(self.e)
        self.kw = dict(decay=decay, every=every, start_step=start_step, warmup=warmup)

    def step(self, p, t, e_device_before=None):
        """`e_device_before`: the device's own average before this write, if read back — the bound takes the larger magnitude"""
        before = self.e
        new, wrote, copied = update(self.e, p, t, **self.kw)
        if copied:
            self.bound = np.zeros_like(self.bound)
        elif wrote:
            mag = before if e_device_before is None else np.maximum(np.abs(before), np.abs(np.asarray(e_device_before, dtype=np.float64)))
            self.bound = self.bound + bound_term(mag, p)
        self.e = new
        return wrote
