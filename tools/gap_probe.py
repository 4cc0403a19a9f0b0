#!/usr/bin/env python3
"""What per-read chaining gaps save a caller with reads of mixed lengths: a seeded batch of trimmed `sr` pairs (tests/gap_model.py's
scenario: mates of 30..150 bases, so almost every pair has its own gaps) mapped twice on one GPU,
  grouped   as a caller had to before chaindp_set_read_gaps: chaindp_map_frag_seqs once per distinct (gap_ref, gap_qry) pair, with the
            package and library of a built checkout of the commit before (PARENT_ROOT);
  one_call  in one chaindp_map_frag_seqs call with gaps=, on this build.
Each runs in a process of its own: one warm-up, then five repetitions, the median wall time of a repetition is the figure.  The reads'
bases, index and options are the same; the grouped side's packing of each group's bases is done before the clock starts.
  python tools/gap_probe.py both PARENT_ROOT [n_pairs=20000] [out=profiles/gap_probe.json]     starts the two runs and writes the record
  python tools/gap_probe.py grouped|one_call [n_pairs]                                         one side; the last line is its JSON"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
REPS = 5


def side(mode, n_pairs):
    sys.path.insert(0, os.path.join(ROOT, "tests"))                  # the scenario and its helpers are this checkout's on either side
    sys.path.insert(0, os.environ.get("GAP_PROBE_PACKAGE_ROOT") or ROOT)
    import frag_model as fm
    import gap_model as gm
    from minimap2_chaindp_amd import chaindp, params as P
    sc = gm.scenario(n_frags=n_pairs, seed=11)
    grp = gm.groups(sc)
    seq, seq_off, ns = fm.batch(sc.frags)
    packed = []
    for (gr, gq), sel in grp:
        par = P.ChainParams(*sc.par.astuple())
        par.max_dist_x, par.max_dist_y = gr, gq
        packed.append((par, fm.batch([sc.frags[r] for r in sel]), sc.bid[sel], sc.hash_[sel]))
    with chaindp.Device(0, max_anchors=max(1 << 22, n_pairs * 400), max_reads=n_pairs + 16) as dev:
        ix = dev.load_index(sc.image())
        args = (ix, sc.w, sc.k, sc.hpc, sc.flag, sc.max_occ)

        def grouped():
            hits = 0
            for par, (s, so, n), bid, hash_ in packed:
                hits += len(dev.map_frag_seqs(*args, par, sc.min_cnt, sc.opt, s, so, n, bid, hash_, sc.ref_len, pe_ori=sc.pe_ori)[1])
            return hits

        def one_call():
            return len(dev.map_frag_seqs(*args, sc.par, sc.min_cnt, sc.opt, seq, seq_off, ns, sc.bid, sc.hash_, sc.ref_len, pe_ori=sc.pe_ori, gaps=sc.gaps)[1])

        fn = grouped if mode == "grouped" else one_call
        hits = fn()                                                   # warm-up: buffers grow, code objects load
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"mode": mode, "reads": n_pairs, "segments": int(ns.sum()), "bases": int(len(seq)), "gap_groups": len(grp), "calls_per_repetition": len(grp) if mode == "grouped" else 1,
           "final_hits": int(hits), "ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3)}
    print(json.dumps(rec))


def both(parent_root, n_pairs, out):
    recs = {}
    for mode, lib in (("grouped", parent_root), ("one_call", None)):
        env = dict(os.environ)
        env.pop("CHAINDP_LIB", None)
        env.pop("GAP_PROBE_PACKAGE_ROOT", None)
        if lib:
            env["GAP_PROBE_PACKAGE_ROOT"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(n_pairs)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{mode} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        recs[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        recs[mode]["build"] = "the parent commit's" if lib else "this one"
    a, b = recs["grouped"], recs["one_call"]
    rec = {"probe": "gap_probe", "reads": a["reads"], "segments": a["segments"], "bases": a["bases"], "gap_groups": a["gap_groups"], "repetitions": REPS,
           "grouped_median_ms": a["median_ms"], "one_call_median_ms": b["median_ms"], "same_final_hits": a["final_hits"] == b["final_hits"],
           "grouped": a, "one_call": b}
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: rec[k] for k in ("reads", "gap_groups", "grouped_median_ms", "one_call_median_ms", "same_final_hits")}))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("both", "grouped", "one_call") or (sys.argv[1] == "both" and len(sys.argv) < 3):
        sys.exit(__doc__)
    if sys.argv[1] == "both":
        both(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20000, sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "gap_probe.json"))
    else:
        side(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
