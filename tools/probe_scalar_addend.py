"""`sin(fmadd(gather(A, i), x, c))` with a host scalar c next to the shapes it should cost the same as: 64 Mi lookups into K = 1 Mi
entries, forward + backward() per step, one process.  GPU box:

    python tools/probe_scalar_addend.py [label [only]]

    (a) hsum(sin(fmadd(gather(A, i), x, c)))               the scalar addend
    (b) hsum(sin(gather(A, i) * x))                        the product alone: the same kernels over the same bytes
    (c) hsum(sin(fmadd(gather(A, i), x, gather(B, i))))    the headline's two-table step

Every shape runs a few steps first (allocator, clocks), then the shapes are timed in the order a b c a b: one line per measurement
(best / worst of three timed regions of five steps) and one with the step's kernels.  `label` names the
library under test in an A/B run (the libraries are swapped between processes: with a library that predates the scalar entry
point (a) runs in element order); `only` names the shapes to time instead, in order (a, or acac)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enoki_amd import capi, hiprt, synth  # noqa: E402
import enoki_amd.hip_autodiff as ad  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "-"
only = sys.argv[2] if len(sys.argv) > 2 else None
capi.init(); st = capi.stream()
n, K, c = 1 << 26, 1 << 20, 0.5
A0, B0 = synth.uniform_pm1(0, K, 6), synth.uniform_pm1(0, K, 7)
x, idx = ad.Float32(synth.uniform_pm1(0, n, 2)), ad.UInt32(synth.index_mod(0, n, 4, K))
out = {}


def step(shape):
    A = ad.Float32(A0)
    ad.set_requires_gradient(A)
    if shape == "c":                       # (both leaves before both gathers, as bench.py records them: the sweep then
        B = ad.Float32(B0)                 #  meets the two gather nodes next to each other and scatters them together)
        ad.set_requires_gradient(B)
    a = ad.gather(A, idx)
    if shape == "a":
        u = ad.fmadd(a, x, ad.Float32(c))
    elif shape == "b":
        u = a * x
    else:
        u = ad.fmadd(a, x, ad.gather(B, idx))
    y = ad.hsum(ad.sin(u))
    ad.backward(y)
    out["y"], out["gA"] = ad.detach(y), ad.gradient(A)
    if shape == "c":
        out["gB"] = ad.gradient(B)


def kernels(fn):
    """one step's kernels by name: launches, and HIP-event time per launch (a delta includes the gap to the previous launch)"""
    ad.hip_profile_begin()
    fn()
    prof = [k for k in json.loads(ad.hip_profile_end()) if k["launches"]]
    return ", ".join(f"{k['kernel']} {k['launches']} x {k['total_ms'] / k['launches'] * 1e3:.1f} us" for k in prof), len(prof)


NAMES = {"a": "(a) sin(fmadd(gather(A,i), x, c))", "b": "(b) sin(gather(A,i) * x)", "c": "(c) sin(fmadd(gather(A,i), x, gather(B,i)))"}
shapes = only if only else "abcab"
for shape in sorted(set(shapes)):
    for _ in range(5):
        step(shape)
for shape in shapes:
    f = lambda: step(shape)
    ms = [hiprt.time_region(st, f, iters=5, warmup=2) for _ in range(3)]
    line, _ = kernels(f)
    order = "bucket order" if "bucket_partition" in line else "element order"
    print(f"{label:8s} {NAMES[shape]:44s} n=2^26 K=2^20  best {min(ms):7.3f} ms  worst {max(ms):7.3f} ms  "
          f"{n / min(ms) / 1e6:6.1f} Gelem/s  {order}  y = {float(out['y'].numpy()[0]):.6g}", flush=True)
    print("         " + line, flush=True)
