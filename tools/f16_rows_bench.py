"""Half-width rows in the graph (HNSWIndex(row_dtype="f16")) against f32 rows, same graph.

python tools/f16_rows_bench.py [--n 200000] [--dims 384,768] [--batch 1024] [--ef 50] [--seconds 2.0] [--out FILE]

Per dimension the same graph is built twice, on the device, from rows that are fp16-representable (so both stores hold
identical values and the two graphs must come out identical: checked), and for each store this prints
  store_bytes         HBM held by the rows
  inserts_per_s       the whole build, one batch_insert call (upload, bookkeeping and linking), and a 2048-row batch into
                      the finished graph
  queries_per_s       device traversal, k 10, batches of --batch queries resident in HBM, ef --ef: wall clock around
                      search_dev calls (each ends with the results on the host), the two stores ALTERNATING in rounds of
                      --seconds each, three rounds apiece after a warm-up round; every round is printed, the spread
                      between rounds of one store is the noise to read a difference against
One JSON line per dimension at the end (and into --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fvdb_import  # noqa: E402


def build(fv, ctx, x, xt, levels, tlevels, a, row_dtype):
    n = x.shape[0]
    g = fv.HNSWIndex(ctx, a.m, a.m0, a.efc, seed=42, row_dtype=row_dtype)
    t0 = time.time()
    assert g.batch_insert(np.arange(n, dtype=np.uint64), x, levels) == (n, 0)
    t1 = time.time()
    assert g.batch_insert(np.arange(n, n + xt.shape[0], dtype=np.uint64), xt, tlevels) == (xt.shape[0], 0)
    t2 = time.time()
    return g, n / (t1 - t0), xt.shape[0] / (t2 - t1)


def one_round(g, q_dev, B, d, ef, seconds):
    """searches of the batches in turn for about `seconds`; queries per second"""
    done, i = 0, 0
    t0 = time.time()
    while True:
        g.search_dev(q_dev[i % len(q_dev)], B, d, 10, ef)
        done += B
        i += 1
        el = time.time() - t0
        if el >= seconds:
            return done / el


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dims", default="384,768")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--m0", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ef", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--tail", type=int, default=2048)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fv = fvdb_import.load()
    import oracle as orc
    from _data import mixture
    orc.build()
    ctx = fv.Context(0)
    lines = []
    for d in [int(s) for s in a.dims.split(",")]:
        x = mixture(a.n + a.tail, d, n_comp=4096, sigma=0.35, seed=1234).astype(np.float16).astype(np.float32)
        x, xt = x[:a.n], x[a.n:]
        levels, tlevels = orc.rng_levels(42, a.n), orc.rng_levels(43, a.tail)
        q = mixture(8 * a.batch, d, n_comp=4096, sigma=0.35, seed=99)  # queries are f32 and not rounded
        q_dev = [ctx.upload(q[i * a.batch:(i + 1) * a.batch]) for i in range(8)]
        res = {"n": a.n, "d": d, "M": a.m, "M0": a.m0, "ef_construction": a.efc, "batch": a.batch, "ef": a.ef, "k": 10}
        idx = {}
        for dt in ("f32", "f16"):
            g, build_rate, tail_rate = build(fv, ctx, x, xt, levels, tlevels, a, dt)
            st = g.insert_stats()
            idx[dt] = g
            res[dt] = {"store_bytes": g.store_bytes(), "build_inserts_per_s": round(build_rate), "tail_inserts_per_s": round(tail_rate),
                       "host_path_inserts": st["host_path_inserts"], "queries_per_s_rounds": []}
            print(f"[build] d {d} {dt}: {a.n} nodes at {build_rate:.0f} inserts/s, then {a.tail} more at {tail_rate:.0f} inserts/s; "
                  f"store_bytes {g.store_bytes()}; host-path inserts {st['host_path_inserts']}", flush=True)
        ga, gb = idx["f32"].export_graph(), idx["f16"].export_graph()
        same = all(np.array_equal(u, v) for u, v in zip(ga, gb)) and idx["f32"].entry_point() == idx["f16"].entry_point()
        r32, r16 = idx["f32"].search_dev(q_dev[0], a.batch, d, 10, a.ef), idx["f16"].search_dev(q_dev[0], a.batch, d, 10, a.ef)
        same_hits = np.array_equal(r32.ids, r16.ids) and np.array_equal(r32.distances.view(np.uint32), r16.distances.view(np.uint32))
        res["same_graph"], res["same_results"] = bool(same), bool(same_hits)
        print(f"[check] d {d}: graphs identical {same}, first batch's ids and distance bits identical {same_hits}", flush=True)
        assert same and same_hits
        del ga, gb
        for rnd in range(4):  # round 0 warms both up
            for dt in ("f32", "f16"):
                rate = one_round(idx[dt], q_dev, a.batch, d, a.ef, a.seconds if rnd else 0.5)
                if rnd:
                    res[dt]["queries_per_s_rounds"].append(round(rate))
                    print(f"[traversal] d {d} {dt} round {rnd}: {rate:.0f} queries/s", flush=True)
        for dt in ("f32", "f16"):
            res[dt]["device_fallbacks"] = idx[dt].device_fallbacks()
        for p in q_dev:
            ctx.free(p)
        idx.clear()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
