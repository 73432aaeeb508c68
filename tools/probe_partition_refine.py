"""The refined stream of a kept bucket partition (csrc/ek_refine.h, bucket_refine.hip): the cfg3b step on a kept partition with the
stream (tuning `partition_refine` = 2) against the same step on the partition's pages (= 0), alternated inside ONE process over
their own (x, index) arrays; what the one-time refinement costs (the first hit against a later one) and what it pins (live bytes).

    python tools/probe_partition_refine.py [log2 n ...] [--steps 200] [--zipf] [--tag text]

The density sweep of DESIGN section 6 is `probe_partition_refine.py 22 23 24 26` (4, 8, 16 and 64 lookups per entry of 1 Mi)."""
import gc, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import enoki_amd.hip_autodiff as ek
from enoki_amd import synth
import enoki_amd.hip as ekc

args = sys.argv[1:]
steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 200
tag = args[args.index("--tag") + 1] if "--tag" in args else "new"
zipf = "--zipf" in args
logns = []
for a in args:                                            # the sizes come first
    if a.startswith("--"):
        break
    logns.append(int(a))
logns = logns or [26]
ek.hip_init(0)
K = 1 << 20
A0, B0 = synth.uniform_pm1(0, K, 6), synth.uniform_pm1(0, K, 7)


def live_bytes():
    gc.collect()
    return int(re.search(r"live bytes\s*:\s*(\d+)", ek.hip_whos()).group(1))


def make(n):
    x = ek.Float32(synth.uniform_pm1(0, n, 2))
    if zipf:
        m = synth.hash_u32(0, n, 8) % ekc.UInt32(20)
        lo = (ekc.UInt32(1) << m) - ekc.UInt32(1)
        idx = ek.UInt32(lo + (synth.hash_u32(0, n, 9) & lo))
    else:
        idx = ek.UInt32(synth.index_mod(0, n, 4, K))
    return x, idx


def step(x, idx):
    A = ek.Float32(A0); B = ek.Float32(B0)
    ek.set_requires_gradient(A); ek.set_requires_gradient(B)
    y = ek.hsum(ek.sin(ek.fmadd(ek.gather(A, idx), x, ek.gather(B, idx))))
    ek.backward(y)
    return ek.detach(y), ek.gradient(A), ek.gradient(B)


def timed(x, idx, count):
    ek.hip_sync()
    t0 = time.perf_counter()
    for _ in range(count):
        r = step(x, idx)
    ek.hip_sync()
    return (time.perf_counter() - t0) / count * 1e3


for logn in logns:
    n = 1 << logn
    modes = {}
    for mode in (0, 2):
        ek.hip_set_tuning("partition_refine", mode)
        before = live_bytes()
        x, idx = make(n)
        arrays = live_bytes() - before
        timed(x, idx, 1)                                  # the partition
        kept = live_bytes() - before - arrays
        first_hit = timed(x, idx, 1)                      # mode 2: the refinement + a step
        pinned = live_bytes() - before - arrays
        timed(x, idx, 20)
        modes[mode] = dict(x=x, idx=idx, first_hit=first_hit, kept=kept, pinned=pinned, ms=[])
    for rep in range(3):
        for mode in (0, 2, 2, 0):
            ek.hip_set_tuning("partition_refine", mode)
            modes[mode]["ms"].append(timed(modes[mode]["x"], modes[mode]["idx"], steps))
    p, r = modes[0], modes[2]
    fmt = lambda v: " ".join(f"{m:.4f}" for m in v)
    print(f"{tag:8s} n = 2^{logn} ({n // K} per entry{', zipf' if zipf else ''})  pages: {fmt(p['ms'])}   refined: {fmt(r['ms'])} ms/step   "
          f"first hit {p['first_hit']:.3f} / {r['first_hit']:.3f} ms   pinned {p['pinned'] / 2**20:.1f} / {r['pinned'] / 2**20:.1f} MiB", flush=True)
    del modes, p, r, x, idx
ek.hip_set_tuning("partition_refine", 1)
