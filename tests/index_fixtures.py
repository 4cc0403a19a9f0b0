"""CHECKER ONLY: the cases of the index-build tiers.  Three fixtures of tests/golden/index (make_index_golden.py) and the five seed
fixtures of tests/golden/seeds whose targets lie in tests/golden/fa; every case carries the reference's image in canonical form
(index_build_model.canonical).  The model's image of a case is built once and shared."""
import functools
import os

import numpy as np

import index_build_model as ibm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX_CASES = ("dense_mapont", "dense_avapb", "heavy_buckets")
# seed fixture -> (target FASTA, w, k, is_hpc, mid_occ comes from mm_idx_cal_max_occ); sr sets mid_occ = 1000 itself (options.c:130)
SEED_CASES = {"mt_orang_vs_human_mapont": ("MT-human.fa", 10, 15, 0, True), "mt_human_vs_orang_avaont": ("MT-orang.fa", 5, 15, 0, True),
              "mt_human_self_avaont": ("MT-human.fa", 5, 15, 0, True), "inv_mapont": ("t-inv.fa", 10, 15, 0, True),
              "inv_sr": ("t-inv.fa", 11, 21, 0, False)}
CASES = INDEX_CASES + tuple(SEED_CASES)
MID_OCC_FRAC = 2e-4            # mm_mapopt_init, options.c:26


def read_fasta(path):
    names, seqs = [], []
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode())
            seqs.append(bytearray())
        elif seqs:
            seqs[-1] += line.strip()
    return names, [bytes(s) for s in seqs]


def name_ranks(names):
    order = sorted(range(len(names)), key=lambda i: names[i].encode())
    rank = np.zeros(len(names), np.uint32)
    rank[order] = np.arange(len(names))
    return rank


@functools.lru_cache(maxsize=None)
def case(name):
    c = {"name": name, "seeds": None}
    if name in INDEX_CASES:
        g = np.load(os.path.join(GOLDEN, "index", name + ".npz"), allow_pickle=False)
        c.update(seq=g["seq"], seq_off=g["seq_off"], rank=g["rank"], w=int(g["w"]), k=int(g["k"]), is_hpc=int(g["is_hpc"]),
                 mid_occ=int(g["mid_occ"]), min_mid_occ=int(g["min_mid_occ"]))
    else:
        fa, w, k, is_hpc, cal = SEED_CASES[name]
        g = np.load(os.path.join(GOLDEN, "seeds", name + ".npz"), allow_pickle=False)
        names, seqs = read_fasta(os.path.join(GOLDEN, "fa", fa))
        c.update(seq=np.frombuffer(b"".join(seqs), np.uint8), seq_off=np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64),
                 rank=name_ranks(names), w=w, k=k, is_hpc=is_hpc, mid_occ=int(g["mid_occ"]) if cal else None, min_mid_occ=0,
                 seeds={k_: g[k_] for k_ in g.files})
    c["raw"] = [g["img_B"], g["img_H"], g["img_V"], g["img_P"]]
    c["img"] = ibm.canonical(c["raw"])
    c["seqs"] = [c["seq"][c["seq_off"][i]:c["seq_off"][i + 1]] for i in range(len(c["seq_off"]) - 1)]
    return c


@functools.lru_cache(maxsize=None)
def model(name):
    """(blobs, route) of the model for a case."""
    c = case(name)
    return ibm.build(ibm.minimizers(c["seqs"], c["w"], c["k"], c["is_hpc"]), c["rank"], 14)
