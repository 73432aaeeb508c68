"""The partition cache (include/enoki/hip.h, HIPBuffer::PartitionEntry; ek_hip_bucketed_partition_retain / ek_hip_bucketed_pair_create_on):
the bucket partition of `fmadd(gather(A, idx), x, gather(B, idx))` depends on (idx, x, mask) only, so a step over the SAME index, x
and mask arrays -- the tables change, as in a fit -- stands on the partition of the step before and launches neither
`bucket_partition` nor `bucket_directory`.  Whatever can change the contents of one of the three gives a miss and the result of the
NEW contents; an array whose pointer has been handed out is never trusted again.

n = 300 007 lookups (odd, above the 2^18 floor of the bucket-ordered path) into K = 65 536 entries: the smallest shape that takes the
hinted fixed-point forward + adjoint kernel of the headline step.  Launches are counted with hip_profile_begin / hip_profile_end.
References: conftest.cfg3b_truth / cfg3b_variant_truth (float64, class-D bounds), eager evaluation for element values, and -- the
fixed-point sums being exact integers -- bit equality with a step on fresh handles with the cache switched off.

(The python modules bind no scatter into a mask array: the mask's contents change through the data_ptr() refill, and the mask comes,
goes and is replaced; tests/cpp/partition_cache_host.cpp writes into it.)"""
import ctypes
import gc
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import bits_equal, cfg3b_truth, cfg3b_variant_truth

pytestmark = pytest.mark.gpu

N, K = 300007, 65536
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ad():
    import enoki_amd.hip_autodiff as m
    m.hip_init(0)
    return m


_HOST = {}


def host(seed=1, k=K):
    """inputs and their float64 truth, computed once per (seed, table size) and never modified"""
    if (seed, k) not in _HOST:
        rng = np.random.default_rng(1000 * seed + 7)
        h = dict(A=rng.uniform(-1, 1, k).astype(np.float32), B=rng.uniform(-1, 1, k).astype(np.float32),
                 x=rng.uniform(-1, 1, N).astype(np.float32), idx=rng.integers(0, k, N).astype(np.uint32),
                 mask=(rng.integers(0, 4, N) != 0))
        for a in h.values():
            a.setflags(write=False)
        _HOST[(seed, k)] = h
    return _HOST[(seed, k)]


def counted(ad, fn):
    ad.hip_profile_begin()
    r = fn()
    prof = json.loads(ad.hip_profile_end())
    return r, {k["kernel"]: k["launches"] for k in prof if k["launches"]}


def step(ad, hA, hB, x, idx, mask=None, form="pair", keep=None):
    """one step of the benchmark's shape over the caller's x / idx / mask arrays and FRESH leaves; -> (y, gA, gB) on the host"""
    A, B = ad.Float32(hA), ad.Float32(hB)
    ad.set_requires_gradient(A); ad.set_requires_gradient(B)
    a = ad.gather(A, idx, mask) if mask is not None else ad.gather(A, idx)
    if form == "pair":
        b = ad.gather(B, idx, mask) if mask is not None else ad.gather(B, idx)
        u = ad.fmadd(a, x, b)
    elif form == "scalar":
        u = ad.fmadd(a, x, ad.Float32(0.5))
    else:
        u = a * x
    if keep is not None:
        keep.append(u)
    y = ad.hsum(ad.sin(u))
    ad.backward(y)
    return ad.detach(y).numpy().copy(), ad.gradient(A).numpy().copy(), (ad.gradient(B).numpy().copy() if form == "pair" else None)


def partitions(ks):
    return ks.get("bucket_partition", 0)


def is_hit(ks):
    return (partitions(ks) == 0 and ks.get("bucket_directory", 0) == 0 and ks.get("bucket_pair_fma_reduce_adjoint", 0) == 1 and
            ks.get("scatter_add_fold", 0) == 1)


def within_truth(r, t, what=("y", "gA", "gB")):
    y, gA, gB = r
    ok = True
    if "y" in what:
        ok = ok and abs(float(y[0]) - t["y"]) <= t["y_bound"]
    if "gA" in what:
        ok = ok and bool(np.all(np.abs(gA - t["gA"]) <= t["gA_bound"]))
    if "gB" in what:
        ok = ok and bool(np.all(np.abs(gB - t["gB"]) <= t["gB_bound"]))
    return ok


def same_bits(r, s):
    return all(bits_equal(a, b) for a, b in zip(r, s) if a is not None)


def cache_off_reference(ad, hA, hB, hx, hidx, hmask=None, form="pair"):
    """the step on fresh handles with the cache switched off"""
    ad.hip_set_tuning("partition_cache", 0)
    try:
        return step(ad, hA, hB, ad.Float32(hx), ad.UInt32(hidx), ad.Mask(hmask) if hmask is not None else None, form)
    finally:
        ad.hip_set_tuning("partition_cache", 1)


def refill(capi, arr, h):
    h = np.ascontiguousarray(h)
    capi.check(capi.lib.ek_hip_memcpy_to_device(ctypes.c_void_p(arr.data_ptr()), h.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(h.nbytes)))


def test_second_step_stands_on_the_first_partition(ad):
    h = host(1)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    r1, k1 = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    r2, k2 = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    assert partitions(k1) == 1 and k1.get("bucket_directory", 0) == 1, k1
    assert is_hit(k2), k2
    assert same_bits(r1, r2)
    assert within_truth(r1, cfg3b_truth(h["A"], h["B"], h["x"], h["idx"]))


def test_tables_change_between_steps(ad):
    h, h2 = host(1), host(2)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    step(ad, h["A"], h["B"], x, idx)
    r2, k2 = counted(ad, lambda: step(ad, h2["A"], h2["B"], x, idx))           # the optimiser's update: other tables, same lookups
    assert is_hit(k2), k2
    assert within_truth(r2, cfg3b_truth(h2["A"], h2["B"], h["x"], h["idx"]))
    assert same_bits(r2, cache_off_reference(ad, h2["A"], h2["B"], h["x"], h["idx"]))


CHANGES = ["scatter_idx", "scatter_idx_aliased", "scatter_x", "scatter_x_aliased", "refill_idx", "refill_x", "refill_mask", "torch_x",
           "other_x", "add_mask", "remove_mask"]


@pytest.mark.parametrize("change", CHANGES)
def test_changed_contents_are_a_miss(ad, capi, change):
    h, h2 = host(1), host(3)
    hx, hidx, hmask = h["x"].copy(), h["idx"].copy(), h["mask"].copy()
    masked = change in ("refill_mask", "remove_mask")
    x, idx = ad.Float32(hx), ad.UInt32(hidx)
    mask = ad.Mask(hmask) if masked else None
    step(ad, h["A"], h["B"], x, idx, mask)
    _, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, mask))
    assert is_hit(k), k
    sticky = False
    pos = np.arange(0, N, 7, dtype=np.uint32)
    aliased = change.endswith("_aliased")
    if aliased:
        ad.hip_set_scatter_aliasing(True)
    try:
        if change.startswith("scatter_idx"):
            hidx[pos] = h2["idx"][pos]
            ad.scatter(idx, ad.UInt32(h2["idx"][pos]), ad.UInt32(pos))
        elif change.startswith("scatter_x"):
            hx[pos] = h2["x"][pos]
            ad.scatter(x, ad.Float32(h2["x"][pos]), ad.UInt32(pos))
        elif change == "refill_idx":
            hidx = h2["idx"]; refill(capi, idx, hidx); sticky = True
        elif change == "refill_x":
            hx = h2["x"]; refill(capi, x, hx); sticky = True
        elif change == "refill_mask":
            hmask = h2["mask"]; refill(capi, mask, hmask.astype(np.uint8)); sticky = True
        elif change == "torch_x":
            import torch
            t = x.torch()                               # a zero-copy view: whoever holds it may write
            hx = h2["x"]
            t.copy_(torch.from_numpy(hx.copy()))
            torch.cuda.synchronize()
            sticky = True
        elif change == "other_x":
            hx = h2["x"]; x = ad.Float32(hx)
        elif change == "add_mask":
            mask = ad.Mask(hmask); masked = True
        else:
            mask = None; masked = False
        r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, mask))
    finally:
        if aliased:
            ad.hip_set_scatter_aliasing(False)
    assert not is_hit(k) and (partitions(k) == 1 or change == "torch_x"), k       # (an exported x: no bucket order at all)
    t = cfg3b_variant_truth(h["A"], h["B"], hx, hidx, mask=hmask if masked else None)
    assert within_truth(r, t)
    if change != "torch_x":
        assert same_bits(r, cache_off_reference(ad, h["A"], h["B"], hx, hidx, hmask if masked else None))
    if sticky:
        # a pointer went out: every later step partitions for itself
        for _ in range(2):
            r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, mask))
            assert not is_hit(k) and (partitions(k) == 1 or change == "torch_x"), k
            assert within_truth(r, t)


def test_key_mismatches_and_shared_forms(ad):
    h = host(1)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    step(ad, h["A"], h["B"], x, idx)
    # the partition does not depend on the op: a host-scalar addend and the product alone stand on the two-table form's
    r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, form="scalar"))
    assert is_hit(k), k
    assert within_truth(r, cfg3b_truth(h["A"], np.full(K, 0.5, np.float32), h["x"], h["idx"]), ("y", "gA"))
    r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx, form="product"))
    assert is_hit(k), k
    assert within_truth(r, cfg3b_variant_truth(h["A"], h["B"], h["x"], h["idx"], spelling="a*x"), ("y", "gA"))
    # another table size over the same (idx, x): a miss
    big = host(4, 2 * K)
    r, k = counted(ad, lambda: step(ad, big["A"], big["B"], x, idx))
    assert partitions(k) == 1, k
    assert within_truth(r, cfg3b_truth(big["A"], big["B"], h["x"], h["idx"]))
    # hmax(u): no hint, full-size buckets -- another partition than the hinted hsum(sin(u))'s
    step(ad, h["A"], h["B"], x, idx)
    dA, dB = ad.Float32(h["A"]), ad.Float32(h["B"])
    ad.hip_set_defer(False)
    try:
        u_ref = ad.detach(ad.fmadd(ad.gather(dA, idx), x, ad.gather(dB, idx))).numpy()
    finally:
        ad.hip_set_defer(True)
    m, k = counted(ad, lambda: ad.detach(ad.hmax(ad.fmadd(ad.gather(dA, idx), x, ad.gather(dB, idx)))).numpy())
    assert partitions(k) == 1, k
    assert bits_equal(m, np.array([u_ref.max()]))
    m, k = counted(ad, lambda: ad.detach(ad.hmax(ad.fmadd(ad.gather(dA, idx), x, ad.gather(dB, idx)))).numpy())
    assert partitions(k) == 0 and bits_equal(m, np.array([u_ref.max()])), k
    # a 64-bit index array: narrowed once, and the partition sits on the narrowed copy
    idx64 = ad.UInt64(idx)
    r1, k1 = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx64))
    r2, k2 = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx64))
    assert partitions(k1) == 1 and is_hit(k2), (k1, k2)
    t = cfg3b_truth(h["A"], h["B"], h["x"], h["idx"])
    assert within_truth(r1, t) and same_bits(r1, r2)


def test_two_live_users_of_one_partition(ad):
    h, h2 = host(1), host(2)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    dA, dB = ad.Float32(h["A"]), ad.Float32(h["B"])
    ad.hip_set_defer(False)
    try:
        u_ref = ad.detach(ad.fmadd(ad.gather(dA, idx), x, ad.gather(dB, idx))).numpy()
    finally:
        ad.hip_set_defer(True)
    step(ad, h2["A"], h2["B"], x, idx)
    held = []
    step(ad, h["A"], h["B"], x, idx, keep=held)                                  # step N: its u stays in a handle
    r, k = counted(ad, lambda: step(ad, h2["A"], h2["B"], x, idx))               # step N + 1 on the same partition
    assert is_hit(k), k
    assert within_truth(r, cfg3b_truth(h2["A"], h2["B"], h["x"], h["idx"]))
    assert bits_equal(ad.detach(held[0]).numpy(), u_ref)


def captured_launches(ad, h, x, idx, out):
    def body():
        A, B = ad.Float32(out["A0"]), ad.Float32(out["B0"])
        ad.set_requires_gradient(A); ad.set_requires_gradient(B)
        y = ad.hsum(ad.sin(ad.fmadd(ad.gather(A, idx), x, ad.gather(B, idx))))
        ad.backward(y)
        out["y"], out["gA"], out["gB"] = ad.detach(y), ad.gradient(A), ad.gradient(B)
    ad.hip_graph_begin()
    body()
    return ad.hip_graph_end()


def test_capture_after_a_cached_step(ad, capi):
    h, h2 = host(1), host(3)
    # the same capture with the cache off: what a captured step launches
    ad.hip_set_tuning("partition_cache", 0)
    try:
        x0, idx0 = ad.Float32(h["x"]), ad.UInt32(h["idx"])
        out0 = {"A0": ad.Float32(h["A"]), "B0": ad.Float32(h["B"])}
        step(ad, h["A"], h["B"], x0, idx0)
        g0 = captured_launches(ad, h, x0, idx0, out0)
        expected = ad.hip_graph_launch_count(g0)
        ad.hip_graph_destroy(g0)
        del out0, x0, idx0
    finally:
        ad.hip_set_tuning("partition_cache", 1)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    out = {"A0": ad.Float32(h["A"]), "B0": ad.Float32(h["B"])}
    step(ad, h["A"], h["B"], x, idx)
    _, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    assert is_hit(k), k
    g = captured_launches(ad, h, x, idx, out)
    try:
        assert ad.hip_graph_launch_count(g) == expected          # the partition is part of the graph
        ad.hip_graph_launch(g)
        assert within_truth((out["y"].numpy(), out["gA"].numpy(), out["gB"].numpy()), cfg3b_truth(h["A"], h["B"], h["x"], h["idx"]))
        refill(capi, idx, h2["idx"])
        ad.hip_graph_launch(g)
        t2 = cfg3b_truth(h["A"], h["B"], h["x"], h2["idx"])
        assert within_truth((out["y"].numpy(), out["gA"].numpy(), out["gB"].numpy()), t2)
    finally:
        ad.hip_graph_destroy(g)
    r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    assert partitions(k) == 1 and within_truth(r, t2), k


def test_switch_off_partitions_every_step(ad):
    h = host(1)
    x, idx = ad.Float32(h["x"]), ad.UInt32(h["idx"])
    ad.hip_set_tuning("partition_cache", 0)
    try:
        for _ in range(3):
            r, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
            assert partitions(k) == 1 and k.get("bucket_directory", 0) == 1, k
    finally:
        ad.hip_set_tuning("partition_cache", 1)
    step(ad, h["A"], h["B"], x, idx)
    r2, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, idx))
    assert is_hit(k) and same_bits(r, r2), k


ENV_SCRIPT = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import enoki_amd.hip_autodiff as ad
ad.hip_init(0)
rng = np.random.default_rng(1)
n, K = {n}, {k}
hA, hB = rng.uniform(-1, 1, K).astype(np.float32), rng.uniform(-1, 1, K).astype(np.float32)
x, idx = ad.Float32(rng.uniform(-1, 1, n).astype(np.float32)), ad.UInt32(rng.integers(0, K, n).astype(np.uint32))
counts = []
for _ in range(3):
    ad.hip_profile_begin()
    A, B = ad.Float32(hA), ad.Float32(hB)
    ad.set_requires_gradient(A); ad.set_requires_gradient(B)
    y = ad.hsum(ad.sin(ad.fmadd(ad.gather(A, idx), x, ad.gather(B, idx))))
    ad.backward(y)
    float(ad.detach(y).numpy()[0])
    counts.append(sum(k["launches"] for k in json.loads(ad.hip_profile_end()) if k["kernel"] == "bucket_partition"))
print("PARTITIONS", counts)
"""


def test_environment_switch(tmp_path):
    script = tmp_path / "env_switch.py"
    script.write_text(ENV_SCRIPT.format(root=ROOT, n=N, k=K))
    seen = {}
    for value in ("0", "1"):
        env = dict(os.environ, ENOKI_HIP_PARTITION_CACHE=value)
        out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        seen[value] = re.search(r"PARTITIONS (\[.*\])", out.stdout).group(1)
    assert seen["0"] == "[1, 1, 1]" and seen["1"] == "[1, 0, 0]", seen


def live_bytes(ad):
    gc.collect()
    return int(re.search(r"live bytes\s*:\s*(\d+)", ad.hip_whos()).group(1))


@pytest.mark.parametrize("which", ["idx", "x", "mask"])
def test_partition_dies_with_its_arrays(ad, which):
    h = host(1)
    # (what the context keeps for itself -- counter blocks, reduction scratch -- exists after one step on other arrays)
    step(ad, h["A"], h["B"], ad.Float32(h["x"]), ad.UInt32(h["idx"]), ad.Mask(h["mask"]))
    base = live_bytes(ad)
    arrays = {}
    sizes = {}
    for name, make in (("x", lambda: ad.Float32(h["x"])), ("idx", lambda: ad.UInt32(h["idx"])), ("mask", lambda: ad.Mask(h["mask"]))):
        before = live_bytes(ad)
        arrays[name] = make()
        sizes[name] = live_bytes(ad) - before
    with_arrays = live_bytes(ad)
    r = step(ad, h["A"], h["B"], arrays["x"], arrays["idx"], arrays["mask"])
    r, k = counted(ad, lambda: step(ad, h["A"], h["B"], arrays["x"], arrays["idx"], arrays["mask"]))
    assert is_hit(k), k
    del r
    assert live_bytes(ad) > with_arrays                         # the kept partition
    del arrays[which]
    assert live_bytes(ad) == with_arrays - sizes[which]          # gone with the first of its three arrays
    arrays.clear()
    assert live_bytes(ad) == base


def test_fresh_index_arrays_do_not_accumulate(ad):
    h = host(1)
    x = ad.Float32(h["x"])
    step(ad, h["A"], h["B"], x, ad.UInt32(h["idx"]))
    after_one = live_bytes(ad)
    for s in range(20):
        _, k = counted(ad, lambda: step(ad, h["A"], h["B"], x, ad.UInt32(h["idx"])))
        assert partitions(k) == 1, k
    assert live_bytes(ad) == after_one
