"""The miss path of the partition cache: the cfg3b step with a FRESH index array every step (copies made outside the timed region),
so that every step runs the partition, looks for a kept one, and keeps its own -- against the same step over one index array
(every step after the first stands on the kept partition).  Run it with the product library and with the parent's (which has no
partition entries: the binding then partitions every step) inside one GPU call; the miss path must cost what the parent's step costs.

    python tools/probe_partition_cache.py [log2 n] [steps] [tag]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import enoki_amd.hip_autodiff as ek
from enoki_amd import synth
ek.hip_init(0)
logn = int(sys.argv[1]) if len(sys.argv) > 1 else 26
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
tag = sys.argv[3] if len(sys.argv) > 3 else "product"
n, K = 1 << logn, 1 << 20
A0, B0 = synth.uniform_pm1(0, K, 6), synth.uniform_pm1(0, K, 7)
x = ek.Float32(synth.uniform_pm1(0, n, 2))
idx = ek.UInt32(synth.index_mod(0, n, 4, K))


def step(index):
    A = ek.Float32(A0); B = ek.Float32(B0)
    ek.set_requires_gradient(A); ek.set_requires_gradient(B)
    y = ek.hsum(ek.sin(ek.fmadd(ek.gather(A, index), x, ek.gather(B, index))))
    ek.backward(y)
    return ek.detach(y), ek.gradient(A), ek.gradient(B)


def timed(indices):
    """ms per step over the given index arrays, one step each; the arrays exist before the clock starts"""
    ek.hip_sync()
    l0 = ek.hip_launch_count()
    t0 = time.perf_counter()
    for index in indices:
        r = step(index)
    ek.hip_sync()
    return (time.perf_counter() - t0) / len(indices) * 1e3, (ek.hip_launch_count() - l0) / len(indices)


for _ in range(10):
    step(idx)
batch = 8                                            # fresh arrays per timed batch (n = 2^26: 256 MiB each)
for rep in range(3):
    same_ms, same_l = timed([idx] * steps)
    miss_ms, miss_l, done = 0.0, 0.0, 0
    while done < steps:
        fresh = [ek.UInt32(synth.index_mod(0, n, 4, K)) for _ in range(batch)]   # the same contents in new arrays, made outside the timed region
        ms, l = timed(fresh)
        miss_ms += ms * batch; miss_l += l * batch; done += batch
        del fresh
    print(f"{tag:10s} n = 2^{logn}  same index array: {same_ms:.4f} ms/step ({same_l:.1f} launches)   "
          f"fresh index array per step: {miss_ms / done:.4f} ms/step ({miss_l / done:.1f} launches)", flush=True)
