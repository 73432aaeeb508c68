"""`sin(fmadd(gather(A, i), x, c))` with a host scalar c that REQUIRES A GRADIENT next to the same step with a constant c: 64 Mi lookups
into K = 1 Mi entries, forward + backward() per step, one process.  GPU box:

    python tools/probe_trainable_addend.py [label [only]]

    (a) c a constant host scalar                       the path that existed
    (b) c a host scalar that requires a gradient       gradient(c) = one fold of plane 0 of the early sums (addend_adjoint_fold)
    (c) c a size-1 DEVICE array that requires one      the same, the scalar broadcast on the stream into the object's addend table

The shapes run a few steps first (allocator, clocks), then they are timed in the order a b c a b c: one line per measurement (best /
worst of three timed regions of five steps) and one with the step's kernels.  For (b) a third line gives the bytes the fold of plane 0
read, its HIP-event time and the bandwidth that follows.  `label` names the library under test in an A/B run (the libraries are swapped
between processes: with a library that predates ek_hip_bucketed_addend_adjoint shape (b) runs in element order); `only` names the
shapes to time instead, in order."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enoki_amd import capi, hiprt, synth  # noqa: E402
import enoki_amd.hip_autodiff as ad  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "-"
only = sys.argv[2] if len(sys.argv) > 2 else None
capi.init(); st = capi.stream()
n, K, c = 1 << 26, 1 << 20, 0.5
A0 = synth.uniform_pm1(0, K, 6)
x, idx = ad.Float32(synth.uniform_pm1(0, n, 2)), ad.UInt32(synth.index_mod(0, n, 4, K))
c_dev = ad.Float32(np.array([c], np.float32))
out = {}


def step(shape):
    A, dc = ad.Float32(A0), (ad.Float32(c_dev) if shape == "c" else ad.Float32(c))
    ad.set_requires_gradient(A)
    if shape != "a":
        ad.set_requires_gradient(dc)
    y = ad.hsum(ad.sin(ad.fmadd(ad.gather(A, idx), x, dc)))
    ad.backward(y)
    out["y"], out["gA"] = ad.detach(y), ad.gradient(A)
    out["gc"] = ad.gradient(dc) if shape != "a" else None


def kernels(fn):
    """one step's kernels by name: launches, and HIP-event time per launch (a delta includes the gap to the previous launch)"""
    ad.hip_profile_begin()
    fn()
    prof = [k for k in json.loads(ad.hip_profile_end()) if k["launches"]]
    return ", ".join(f"{k['kernel']} {k['launches']} x {k['total_ms'] / k['launches'] * 1e3:.1f} us" for k in prof), prof


NAMES = {"a": "(a) c constant", "b": "(b) c requires a gradient", "c": "(c) device c, requires one"}
shapes = only if only else "abcabc"
for shape in sorted(set(shapes)):
    for _ in range(5):
        step(shape)
for shape in shapes:
    f = lambda: step(shape)
    ms = [hiprt.time_region(st, f, iters=5, warmup=2) for _ in range(3)]
    line, prof = kernels(f)
    order = "bucket order" if "bucket_partition" in line else "element order"
    gc = f"  gc = {float(out['gc'].numpy()[0]):.6g}" if out["gc"] is not None else ""
    print(f"{label:8s} {NAMES[shape]:28s} n=2^26 K=2^20  best {min(ms):7.3f} ms  worst {max(ms):7.3f} ms  "
          f"{n / min(ms) / 1e6:6.1f} Gelem/s  {order}  y = {float(out['y'].numpy()[0]):.6g}{gc}", flush=True)
    print("         " + line, flush=True)
    for k in prof:
        if k["kernel"] == "addend_adjoint_fold":
            us = k["total_ms"] / k["launches"] * 1e3
            print(f"         addend_adjoint_fold: {k['bytes'] / k['launches'] / 1e6:.2f} MB of per-piece tables in {us:.1f} us "
                  f"(launch gap included) = {k['bytes'] / k['launches'] / us / 1e3:.0f} GB/s", flush=True)
