"""CPU tier: the parts of bench.py that are plain host logic -- the issue-rate ceilings read from the committed calibration runs,
the stored PMC figures (quoted only for the build they were measured on, scaled per anchor to a rank's share at N > 1), the
replay-file writer of the packet-ABI entry, and the strong-scaling cut of the job."""
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from minimap2_chaindp_amd import params as P, shard  # noqa: E402


def test_issue_ceilings_come_from_the_committed_calibration():
    c = bench.issue_ceilings()
    assert c is not None and len(c["files"]) >= 1
    assert 850 < c["valu_full"] < 1100 and 520 < c["valu_half"] < 650 and 500 < c["salu"] < 650      # G wave-instructions/s on MI355X
    assert c["valu_half"] < c["valu_full"]


def test_stored_pmc_is_keyed_on_the_kernel_sources_and_scaled_per_anchor(tmp_path, monkeypatch):
    t = bench.stored_pmc_any()
    assert t is not None and "kernel_source_sha16" in t
    n0 = t["anchors_per_launch"]
    monkeypatch.setattr(bench, "kernel_source_sha16", lambda: t["kernel_source_sha16"])
    same = bench.stored_pmc(n0)
    assert same is not None and "scaled_from_anchors" not in same and same["hbm_bytes_per_launch"] == t["hbm_bytes_per_launch"]
    half = bench.stored_pmc(n0 // 2)
    assert half["scaled_from_anchors"] == n0 and abs(half["hbm_bytes_per_launch"] * 2 - t["hbm_bytes_per_launch"]) < 1e-6 * t["hbm_bytes_per_launch"] + 64
    monkeypatch.setattr(bench, "kernel_source_sha16", lambda: "0" * 16)               # another build of the kernels: nothing is quoted
    assert bench.stored_pmc(n0) is None and bench.measured_traffic(n0) is None and bench.measured_issue(n0, 1.0) is None


def test_replay_file_layout(tmp_path):
    par = P.preset("ava-ont")
    packets = [b"\x01" * 64 + b"\x02" * 128, b"\x03" * 64]
    path = str(tmp_path / "x.rpl")
    bench._replay_file(path, packets, [np.arange(5, dtype=np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8)], 7, 9, par)
    raw = open(path, "rb").read()
    assert raw[:8] == b"SHIMRPL1"
    flag, mid_occ, bw, max_skip, min_sc, n = struct.unpack_from("<6i", raw, 8)
    assert (flag, mid_occ, bw, max_skip, min_sc, n) == (7, 9, par.bw, par.max_skip, par.min_sc, 2)
    pos = 32
    sizes = []
    for _ in range(4):
        (nb,) = struct.unpack_from("<q", raw, pos)
        sizes.append(nb)
        pos += 8 + nb
    assert sizes == [5, 0, 0, 0]
    for pk in packets:
        (sz,) = struct.unpack_from("<I", raw, pos)
        assert sz == len(pk) and raw[pos + 4:pos + 4 + sz] == pk
        pos += 4 + sz
    assert pos == len(raw)


def test_job_cuts_tile_the_job_and_balance_anchors():
    cuts = shard.job_cuts("ava-ont", 4, 64, seed=3, threads=2)
    assert cuts[0] == 0 and cuts[-1] == 64 and np.all(np.diff(cuts) > 0)
    from minimap2_chaindp_amd import anchorgen
    off = anchorgen.offsets("ava-ont", n_reads=64, seed=3, threads=2)
    loads = np.diff(off[cuts])
    assert loads.max() - loads.min() <= 2 * int(np.diff(off).max())
    o, a, first = shard.generate_job_shard("ava-ont", 1, 4, 64, 3, threads=2)
    assert first == int(cuts[1]) and len(o) - 1 == int(cuts[2] - cuts[1]) and int(o[-1]) == int(off[cuts[2]] - off[cuts[1]]) == len(a)


class _FakeResidentBatch:
    """Stands in for a chaindp.Device after bench.py's timed steps: the C calls dump_outputs makes write the given results."""

    def __init__(self, soff, seeds, f, p, v):
        import ctypes as C

        class Lib:
            @staticmethod
            def chaindp_compact_offsets(ctx, par, dst):
                C.memmove(dst, soff.ctypes.data, soff.nbytes)
                return 0

            @staticmethod
            def chaindp_download_seeds(ctx, first, n, dst):
                assert 0 <= first and first + n <= len(seeds)
                C.memmove(dst, seeds[first:].ctypes.data, n * seeds.itemsize)
                return 0

        self._lib, self._ctx, self.fpv = Lib(), None, (f, p, v)

    def _check(self, rc):
        assert rc == 0

    def sync(self):
        pass

    def download(self):
        return tuple(a.copy() for a in self.fpv)


def test_dump_outputs_layout_and_size(tmp_path):
    """bench.py --dump-outputs: float64 files, a fixed sample of whole reads within the size limit, the 64-bit new_seed[] fields
    split so that float64 holds them exactly."""
    from minimap2_chaindp_amd import chaindp
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 9000, 2000)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tot = int(off[-1])
    f, p, v = (rng.integers(-1, 1 << 30, tot).astype(np.int32) for _ in range(3))
    per_read = np.minimum(lens, rng.integers(0, 9000, len(lens)))
    soff = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    seeds = np.zeros(int(soff[-1]), chaindp.SEED_DTYPE)
    seeds["x"] = rng.integers(0, 1 << 63, len(seeds), dtype=np.uint64) | np.uint64(1 << 63)
    seeds["y"] = rng.integers(0, 1 << 63, len(seeds), dtype=np.uint64)
    seeds["p"], seeds["f"] = rng.integers(-1, 1 << 20, len(seeds)), rng.integers(0, 1 << 30, len(seeds))
    par = P.preset("ava-ont")
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), chaindp, _FakeResidentBatch(soff, seeds, f, p, v), par, off)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("seeds_per_read", "sample_reads", "f", "p", "v", "new_seed"))
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:                                                   # same arguments, same files
        assert np.array_equal(np.load(tmp_path / "b" / n), got[n[:-4]])
    assert np.array_equal(got["seeds_per_read"], per_read)
    take = got["sample_reads"].astype(np.int64)
    assert len(take) > 10 and np.all(np.diff(take) > 0) and lens[take].sum() <= bench.DUMP_SAMPLE_ANCHORS
    idx = np.concatenate([np.arange(off[r], off[r + 1]) for r in take])
    for n, a in (("f", f), ("p", p), ("v", v)):
        assert np.array_equal(got[n], a[idx])
    exp = np.concatenate([seeds[soff[r]:soff[r + 1]] for r in take])
    ns = got["new_seed"].astype(np.int64)
    assert ns.shape == (len(exp), 6)
    x = (ns[:, 0].astype(np.uint64) << np.uint64(32)) | ns[:, 1].astype(np.uint64)
    y = (ns[:, 2].astype(np.uint64) << np.uint64(32)) | ns[:, 3].astype(np.uint64)
    assert np.array_equal(x, exp["x"]) and np.array_equal(y, exp["y"])
    assert np.array_equal(ns[:, 4], exp["p"]) and np.array_equal(ns[:, 5], exp["f"])
