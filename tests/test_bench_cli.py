"""bench.py's plain / --full split and --dump-outputs: the argument rules and
the dump helpers on the CPU, and one plain run on the GPU whose dumped arrays
are checked against a direct encode of the same seeded blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def _bench_module(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def test_plain_run_drops_the_side_measurements(monkeypatch):
    bench = _bench_module(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu and a.no_e2e and a.config == "c4"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and not a.no_cpu and not a.no_e2e and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu"])
    a = bench.parse()
    assert a.full and a.no_cpu and not a.no_e2e


def test_block_dump_whole_and_sampled(monkeypatch, tmp_path):
    """Small outputs are dumped whole; past the size limit the samples of a
    fixed, seeded, sorted choice of blocks (the same every call) with every
    block's indices; float32 samples, float64 for the rest, under the limit."""
    bench = _bench_module(monkeypatch, [])
    nb, d = 1000, 8
    idx = torch.arange(nb, dtype=torch.int32).reshape(nb, 1)
    smp = torch.arange(nb * d, dtype=torch.float32)
    out = bench.block_dump(idx, smp, nb, d, 1)
    assert sorted(out) == ["idx", "sample"]
    assert np.array_equal(out["sample"], smp.numpy().reshape(nb, d))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 << 10)
    a = bench.block_dump(idx, smp, nb, d, 1, "_rank1")
    b = bench.block_dump(idx, smp, nb, d, 1, "_rank1")
    assert sorted(a) == ["idx_rank1", "sample_blocks_rank1", "sample_rank1"]
    pick = a["sample_blocks_rank1"]
    assert np.array_equal(pick, b["sample_blocks_rank1"]) and 0 < pick.size < nb
    assert np.all(np.diff(pick) > 0) and pick[0] >= 0 and pick[-1] < nb
    assert np.array_equal(a["sample_rank1"], smp.numpy().reshape(nb, d)[pick])
    assert np.array_equal(a["idx_rank1"], idx.numpy())
    bench.dump_outputs(str(tmp_path / "o"), a)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in os.listdir(tmp_path / "o")}
    assert sorted(got) == sorted(a)
    assert got["sample_rank1"].dtype == np.float32
    assert got["idx_rank1"].dtype == np.float64 and got["sample_blocks_rank1"].dtype == np.float64
    assert np.array_equal(got["idx_rank1"], idx.numpy())
    assert sum(v.nbytes for v in got.values()) <= 16 << 10
    with pytest.raises(SystemExit, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "p"), {"x": np.zeros(3000)})


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_the_timed_step_computed(cwqlib, tmp_path):
    """A plain `bench.py --gpus 1 --steps 2 --warmup 1` on 4,099 C4 blocks: one
    line whose steps is the --steps given, ms_per_step consistent with value,
    the --full fields null, and dumped idx / sample bit-equal to a direct
    encode_blocks of the same seeded blocks."""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    from compression_without_quantization_amd.synthetic import DEFAULT_SEED, make_blocks_range
    nb, d, bits = 4099, 32, 16
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--blocks", str(nb),
                        "--dump-outputs", str(out)],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "blocks/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(nb / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("cpu_baseline", "parity", "pcie_inclusive_blocks_per_s", "decode_blocks_per_s",
              "decode_roundtrip_bit_exact"):
        assert line[k] is None, k
    assert line["roofline"]["kernel_ms"] > 0  # the timed steps' own events
    assert sorted(os.listdir(out)) == ["idx.npy", "sample.npy"]
    idx, smp = np.load(out / "idx.npy"), np.load(out / "sample.npy")
    assert idx.dtype == np.float64 and idx.shape == (nb, 1)
    assert smp.dtype == np.float32 and smp.shape == (nb, d)
    h = make_blocks_range(0, nb, d, bits, seed=DEFAULT_SEED)
    wi, ws = C.encode_blocks(*[h[k].reshape(-1) for k in ("post_loc", "post_scale", "prior_loc",
                                                          "prior_scale")],
                             bits, 1, 42, block_dim=d)
    assert np.array_equal(idx, wi.cpu().numpy().reshape(nb, 1))
    assert np.array_equal(smp.reshape(-1).view(np.uint32), ws.cpu().numpy().view(np.uint32))
