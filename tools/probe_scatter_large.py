"""scatter_add of float32 values into tables beyond 4 Mi bins (the device-sized sliced path): eager time by table size and index
pattern, and the replay of one captured call against the eager call of the same build.  GPU box:

    python tools/probe_scatter_large.py eager [label [pattern]]   64 Mi adds: uniform K=2^24, K=2^26; zipf and all-equal at K=2^24
    python tools/probe_scatter_large.py replay LOGN [label]    K=2^24, 2^LOGN adds: eager call, captured call, replay

One line per measurement and one with the call's kernels; `label` names the library under test in an A/B run (the libraries are swapped between processes)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enoki_amd import capi, hiprt, synth  # noqa: E402
import enoki_amd.hip as ek  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "eager"
capi.init(); st = capi.stream()


def kernels(fn):
    """one call's kernels by name: launches, and HIP-event time per launch (a delta includes the gap to the previous launch)"""
    ek.hip_profile_begin()
    fn()
    prof = [k for k in json.loads(ek.hip_profile_end()) if k["launches"]]
    line = ", ".join(f"{k['kernel']} {k['launches']} x {k['total_ms'] / k['launches'] * 1e3:.1f} us" for k in prof)
    return {k["kernel"]: k["launches"] for k in prof}, line


if mode == "eager":
    label = sys.argv[2] if len(sys.argv) > 2 else "-"
    n = 1 << 26
    vals = synth.uniform_pm1(0, n, 3)
    rng = np.random.default_rng(1)
    only = sys.argv[3] if len(sys.argv) > 3 else None          # one pattern alone
    cases = [("uniform", 24), ("uniform", 26), ("zipf", 24), ("all-equal", 24)]
    for pattern, logk in cases:
        if only and pattern != only:
            continue
        K = 1 << logk
        if pattern == "uniform":
            idx = synth.index_mod(0, n, 4, K)
        elif pattern == "zipf":
            idx = ek.UInt32(((rng.zipf(1.3, n).astype(np.uint64) * 2654435761) % K).astype(np.uint32))
        else:
            idx = ek.UInt32.full(K // 2 + 12345, n)
        t = ek.Float32.zero(K)
        f = lambda: ek.scatter_add(t, vals, idx)
        ms = [hiprt.time_region(st, f, iters=5, warmup=1) for _ in range(3)]
        ks, line = kernels(f)
        path = "device-sized" if "scatter_add_slice_count" in ks else "host-sized"
        print(f"{label:8s} K=2^{logk} {pattern:9s} n=2^26  best {min(ms):8.3f} ms  worst {max(ms):8.3f} ms  "
              f"{n / min(ms) / 1e6:6.1f} G adds/s  {path}, {sum(ks.values())} launches", flush=True)
        print("         " + line, flush=True)
        del idx, t
else:
    logn = int(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else "-"
    n, K = 1 << logn, 1 << 24
    vals = synth.uniform_pm1(0, n, 3)
    idx = synth.index_mod(0, n, 4, K)
    out = {}

    def step():
        t = ek.Float32.zero(K)
        ek.scatter_add(t, vals, idx)
        out["t"] = t

    eager = min(hiprt.time_region(st, step, iters=5, warmup=1) for _ in range(3))
    want = float(ek.hsum(ek.abs(out["t"])).numpy()[0])
    ek.hip_graph_begin()
    try:
        step()
    finally:
        g = ek.hip_graph_end()
    launches = ek.hip_graph_launch_count(g)
    replay = min(hiprt.time_region(st, lambda: ek.hip_graph_launch(g), iters=5, warmup=1) for _ in range(3))
    got = float(ek.hsum(ek.abs(out["t"])).numpy()[0])
    print(f"{label:8s} K=2^24 uniform n=2^{logn}  eager {eager:8.3f} ms  replay {replay:8.3f} ms  ({launches} launches per replay; "
          f"sum |t| eager {want:.6g}, replay {got:.6g})", flush=True)
    ek.hip_graph_destroy(g)
