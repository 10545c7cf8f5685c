"""debug (needs `make -C crossscalepatchmatch_amd/csrc ../libcspm_rowstats.so`; run as a process of its own on the GPU): which leaf of the
row engine's path decision (cspm_rows.h level_rows, counters g_pathstat) every level pass of k_rescore takes on the constructed
cases of tests/rows_path_ref.py, per case, cost source, view and pyramid level.  Prints the histogram (profiles/row_paths.txt) and writes
tests/golden/row_paths.json: the record tests/test_rows_path_ref.py holds the CPU restatement to, with the sha256 of the cspm_rows.h it
was recorded from.  The costs of the counted launches are checked too: DMA-filled and computed tables must give the same bits here, and
their sha256 goes into the record, where tests/test_gpu_row_paths.py holds the CPU oracle's costs to it (tools/ never loads the oracle).

    python tools/row_paths.py [--out tests/golden/row_paths.json]"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["CSPM_LIB"] = os.path.join(ROOT, "crossscalepatchmatch_amd", "libcspm_rowstats.so")
import numpy as np

import crossscalepatchmatch_amd as cs
from crossscalepatchmatch_amd import capi
from crossscalepatchmatch_amd.synth import make_pair
import rows_path_ref as rp

RESCORE_SLOT, SLOTS, LEVELS, LEAVES = 13, 16, 8, 128


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden", "row_paths.json")
    ctx = cs.StereoContext(0)
    L = cs.load_library()
    L.cspm_debug_pathstats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * (2 * SLOTS * LEVELS * LEAVES))()
    record, digests, bad, unlike = {}, {}, 0, 0
    for case in rp.CASES:
        g = case.geom
        l, r, _, _ = make_pair(g.w, g.h, g.max_dis, regions=3, seed=case.seed)
        lam = 0.3 if g.scale_num else 0.0
        fields = rp.case_fields(case)
        ctx.set_images(l, r)
        costs = {}
        for source in ("tables", "computed"):
            ctx.build_cost_grd(g.max_dis, g.wnd, g.scale_num, lam, volumes=False, table_volumes=source == "tables")
            assert ctx.get_option(capi.OPT_TABLE_VOLUMES_ACTIVE) == int(source == "tables")
            for v in (0, 1):
                ctx.set_planes(v, fields[v], np.full((g.h, g.w), -7.0))
            ctx.synchronize()
            assert L.cspm_debug_pathstats(buf, 1) == 0
            ctx.rescore_planes()
            ctx.synchronize()
            assert L.cspm_debug_pathstats(buf, 1) == 0
            a = np.frombuffer(buf, dtype=np.uint64).reshape(2, SLOTS, LEVELS, LEAVES)
            assert a[:, [s for s in range(SLOTS) if s != RESCORE_SLOT]].sum() == 0  # nothing but the re-score ran
            hist = {f"{v}/{s}/{leaf}": int(a[v, RESCORE_SLOT, s, leaf]) for v in (0, 1) for s in range(LEVELS) for leaf in range(LEAVES)
                    if a[v, RESCORE_SLOT, s, leaf]}
            record[f"{case.name}/{source}"] = hist
            costs[source] = [ctx.get_planes(v)[1] for v in (0, 1)]
            for v in (0, 1):
                digests[f"{case.name}/{source}/{v}"] = hashlib.sha256(np.ascontiguousarray(costs[source][v]).tobytes()).hexdigest()
            ok = all(np.array_equal(costs[source][v], costs["tables"][v]) and np.all(costs[source][v] != -7.0) for v in (0, 1))
            bad += not ok
            same = hist == rp.case_histogram(case, source)
            unlike += not same
            print(f"{case.name}/{source}: {g.w}x{g.h} max_dis {g.max_dis} window {g.wnd} levels {g.scale_num}: costs {'== those of the DMA-filled tables' if ok else '!= THOSE OF THE DMA-FILLED TABLES'}, "
                  f"counters {'== restatement' if same else '!= RESTATEMENT'}")
            for key, cnt in hist.items():
                v, s, leaf = (int(t) for t in key.split("/"))
                print(f"    view {v} level {s}: {cnt:5d}  {rp.leaf_name(leaf)}")
    with open(os.path.join(ROOT, "crossscalepatchmatch_amd", "csrc", "cspm_rows.h"), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(out, "w") as f:
        json.dump({"cspm_rows_h_sha256": sha, "tool": "tools/row_paths.py", "cases": record, "min_cost_sha256": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out} ({len(record)} launches, cspm_rows.h {sha[:12]}); {bad} launches whose costs differ between the table sources, "
          f"{unlike} whose counters differ from tests/rows_path_ref.py (a slip in the restatement: the record is what the device did)")
    ctx.close()
    return 1 if bad or unlike else 0


if __name__ == "__main__":
    sys.exit(main())
