"""Sequential HNSW build (HNSWIndex::insert, src/hnsw/core.rs:226-378): the device-resident insert against the CPU
oracle.  python tools/build_bench.py --n 10000 --d 384 [--mode 0|1|2] [--check] [--gen mixture|refbench|latent]
[--visited auto|bitmap|hashed]

Large graphs (the oracle links 200-300 nodes/s: it cannot build them itself):
python tools/build_bench.py --n 1000000 --sample 2048 builds n nodes on the device, installs the exported graph into the
oracle, inserts the next `sample` rows on both and compares every list either of them touched."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fvdb_import  # noqa: E402


def gen(name, n, d, seed):
    from _data import mixture
    if name == "mixture":
        return mixture(n, d, n_comp=4096, sigma=0.35, seed=seed)
    if name == "refbench":
        i = (np.arange(n, dtype=np.int64) + seed).astype(np.float32)
        base = np.fmod(i * np.float32(0.001), np.float32(1.0)).astype(np.float32)
        ramp = (np.arange(d, dtype=np.float32) * np.float32(0.0001)).astype(np.float32)
        return (base[:, None] + ramp[None, :]).astype(np.float32)
    if name == "latent":  # bench.py's generator (C3 headline data)
        import bench
        g = bench.Generator(d=d)
        out = np.empty((n, d), np.float32)
        for c in range(0, n, 10000):
            out[c:c + 10000] = g.rows(min(10000, n - c), stream=c // 10000 + (0 if seed == 1234 else 777))
        return out
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32)


def slot_sums(off, nb):
    """One number per (node, layer) list: its length and an order-sensitive sum of its members."""
    ln = np.diff(off).astype(np.int64)
    pos = np.arange(nb.size, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), ln)
    w = (nb.astype(np.int64) + 1) * (pos + 1)
    cs = np.concatenate([[0], np.cumsum(w)])
    return ln, cs[off[1:].astype(np.int64)] - cs[off[:-1].astype(np.int64)]


def sample_check(gh, orc, a, x, xs, levels):
    """The graph as the device built it goes into the oracle; `sample` more inserts on both; every list the device
    changed, every list of a new node and every list of a node the oracle linked a new node to must be the same."""
    n, k = a.n, xs.shape[0]
    gi, lv, off, nb = gh.export_graph()
    oh = orc.HNSWIndex(a.m, a.m0, a.efc, seed=42)
    t0 = time.time()
    oh.restore(gi, x, lv, off, nb, gh.entry_point())
    print(f"[sample] graph of {n} nodes installed into the oracle ({time.time() - t0:.1f}s)", flush=True)
    ids = np.arange(n, n + k, dtype=np.uint64)
    slv = orc.rng_levels(43, k)
    b = gh.insert_stats()
    t0 = time.time()
    assert gh.batch_insert(ids, xs, slv) == (k, 0)
    t_dev = time.time() - t0
    e = gh.insert_stats()
    t0 = time.time()
    oh.batch_insert(ids, xs, slv)
    t_orc = time.time() - t0
    info = gh.insert_info()
    print(f"[sample] {k} inserts at {n} nodes: device {k / t_dev:.0f} inserts/s ({t_dev / k * 1e3:.3f} ms each), oracle {k / t_orc:.0f} inserts/s; "
          f"representation {info['representation']}, host-path inserts {e['host_path_inserts'] - b['host_path_inserts']}, hashed "
          f"{e['hashed_inserts'] - b['hashed_inserts']}, visited overflows {e['visited_overflows'] - b['visited_overflows']}", flush=True)
    gi2, lv2, off2, nb2 = gh.export_graph()
    slots = off.size - 1
    l0, s0 = slot_sums(off, nb)
    l1, s1 = slot_sums(off2, nb2)
    changed = np.nonzero((l0 != l1[:slots]) | (s0 != s1[:slots]))[0]
    first_slot = np.concatenate([[0], np.cumsum(lv2.astype(np.int64) + 1)])
    node_of = np.searchsorted(first_slot, changed, side="right") - 1
    todo = {(int(nd), int(sl - first_slot[nd])) for nd, sl in zip(node_of, changed)}
    for r in range(n, n + k):
        for layer in range(int(lv2[r]) + 1):
            todo.add((r, layer))
            for o in oh.neighbors(int(gi2[r]), layer):
                if int(lv2[o]) >= layer:  # (a search may start from a node that does not reach this layer, :323)
                    todo.add((int(o), layer))
    bad = 0
    for r, layer in sorted(todo):
        at = int(first_slot[r]) + layer
        if nb2[int(off2[at]):int(off2[at + 1])].tolist() != oh.neighbors(int(gi2[r]), layer):
            if bad < 5:
                print("MISMATCH node", r, "layer", layer)
            bad += 1
    same_entry = gh.entry_point() == oh.entry_point()
    print(f"[sample] lists compared {len(todo)} (changed on the device: {changed.size}), differing from the oracle: {bad}, entry point "
          f"{'same' if same_entry else 'DIFFERENT'}", flush=True)
    assert bad == 0 and same_entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--m0", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--gen", default="mixture")
    ap.add_argument("--check", action="store_true", help="build the same graph with the CPU oracle and compare")
    ap.add_argument("--host", action="store_true", help="host algorithm with per-hop GPU scoring instead")
    ap.add_argument("--chunk", type=int, default=0, help="insert in chunks of this many (0 = one batch_insert call)")
    ap.add_argument("--tail", type=int, default=0, help="after the build: this many more inserts, timed on their own")
    ap.add_argument("--tail-mode", type=int, default=1)
    ap.add_argument("--visited", choices=["auto", "bitmap", "hashed"], default="auto",
                    help="form of the device insert's visited set (HNSWIndex.set_insert_visited)")
    ap.add_argument("--slots", type=int, default=0, help="slots of the hashed visited table (0 = default)")
    ap.add_argument("--sample", type=int, default=0,
                    help="large-graph mode: after the build, this many more inserts on the device and on the oracle "
                         "(which is handed the device's graph), every touched list compared")
    a = ap.parse_args()
    fv = fvdb_import.load()
    import oracle as orc
    orc.build()
    x = gen(a.gen, a.n + a.tail + a.sample, a.d, 1234)
    xs, x = x[a.n + a.tail:], x[:a.n + a.tail]
    xt, x = x[a.n:], x[:a.n]
    ids = np.arange(a.n, dtype=np.uint64)
    levels = orc.rng_levels(42, a.n)
    ctx = fv.Context(0)
    gh = fv.HNSWIndex(ctx, a.m, a.m0, a.efc, seed=42)
    gh.set_device_insert(not a.host, a.mode)
    gh.set_insert_visited(a.visited, a.slots)
    t0 = time.time()
    if a.chunk:
        for o in range(0, a.n, a.chunk):
            gh.batch_insert(ids[o:o + a.chunk], x[o:o + a.chunk], levels[o:o + a.chunk])
            print(f"  {o + a.chunk} nodes {time.time() - t0:.1f}s", flush=True)
    else:
        gh.batch_insert(ids, x, levels)
    t1 = time.time()
    st = gh.insert_stats()
    print(f"[visited] {gh.insert_info()}", flush=True)
    print(f"[build] n {a.n} d {a.d} gen {a.gen} mode {a.mode} visited {a.visited} host {a.host}: {t1 - t0:.2f}s = {a.n / (t1 - t0):.0f} inserts/s "
          f"({(t1 - t0) / a.n * 1e3:.3f} ms each)  stats {st}", flush=True)
    if a.tail:
        gh.set_device_insert(not a.host, a.tail_mode)
        b = gh.insert_stats()
        t0 = time.time()
        gh.batch_insert(np.arange(a.n, a.n + a.tail, dtype=np.uint64), xt, orc.rng_levels(43, a.tail))
        t1 = time.time()
        e = gh.insert_stats()
        print(f"[tail] {a.tail} inserts at {a.n} nodes, mode {a.tail_mode}: {(t1 - t0) / a.tail * 1e3:.3f} ms each; "
              f"{ {k: e[k] - b[k] for k in e} }", flush=True)
    if a.sample:
        assert not a.tail, "--sample compares against a graph exported before the sample: not with --tail"
        sample_check(gh, orc, a, x, xs, levels)
    if a.check:
        t0 = time.time()
        oh = orc.HNSWIndex(a.m, a.m0, a.efc, seed=42)
        oh.batch_insert(ids, x, levels)
        t1 = time.time()
        print(f"[oracle] {t1 - t0:.2f}s = {a.n / (t1 - t0):.0f} inserts/s", flush=True)
        assert gh.entry_point() == oh.entry_point(), (gh.entry_point(), oh.entry_point())
        gi, lv, off, nb = gh.export_graph()
        slot, bad = 0, 0
        for r, l in zip(gi.tolist(), lv.tolist()):
            assert l == oh.level(r)
            for layer in range(l + 1):
                if nb[int(off[slot]):int(off[slot + 1])].tolist() != oh.neighbors(r, layer):
                    if bad < 5:
                        print("MISMATCH node", r, "layer", layer, nb[int(off[slot]):int(off[slot + 1])].tolist(), oh.neighbors(r, layer))
                    bad += 1
                slot += 1
        print(f"[check] lists differing from the oracle: {bad}", flush=True)
        assert bad == 0


if __name__ == "__main__":
    main()
