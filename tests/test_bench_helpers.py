"""bench.py's bookkeeping without a GPU: the committed PMC summary it quotes is parsed, the traffic figure is the profile's bytes per
slot-step scaled to the run's units, and the contract's flags exist with defaults that finish within minutes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _profile_is_stale():
    """The newest committed PMC summary carries the sha256 of the kernel sources it was taken from; between a kernel edit and the next
    profiling run (tools/profile_round.sh on the GPU box) it describes ANOTHER kernel and bench.py must not quote it."""
    rows, source = bench._newest_pmc_rows()
    assert source is not None
    if "stale" in source:
        assert rows == [] and bench.profiled_traffic("ilm::step_lean_kernel<true, false>") is None
        assert bench.profiled_per_wave("ilm::sphere_lights_kernel<0, false, false>", "SQ_INSTS_VALU") is None
        assert bench.step_traffic_fields(None, 5) == {"traffic": None}
        return True
    return False


def test_profiled_traffic_comes_from_the_newest_committed_summary():
    if _profile_is_stale():
        import pytest
        pytest.skip("profiles/*_pmc.csv is older than the kernel sources: bench.py reports null fractions until the round's profile is committed")
    rows, source = bench._newest_pmc_rows()
    assert source is not None and source.endswith("_pmc.csv") and len(rows) > 10
    t = bench.profiled_traffic("ilm::step_lean_kernel<true, false>", "ilm::step_lean_kernel<false, false>")
    assert t is not None and t["lanes"] > 0
    per = t["bytes"] / t["lanes"]
    # one lane per slot: the measured HBM bytes per slot-step are the algorithmic 112 B (padding lanes of partial units pull it down a little)
    assert 100.0 < per < 120.0
    f = bench.step_traffic_fields(t, 2_000_000)
    assert f["traffic"] == round(per * 2_000_000) and abs(f["traffic_per_unit"] - per) < 0.01
    assert f["traffic_profiled"]["slots_per_step"] == round(t["lanes"])
    assert bench.profiled_traffic("ilm::no_such_kernel") is None
    assert bench.step_traffic_fields(None, 5) == {"traffic": None}


def test_light_kernel_instruction_counts_are_in_the_summary():
    if _profile_is_stale():
        import pytest
        pytest.skip("stale profile (see above)")
    for k in ("ilm::sphere_lights_kernel<0, false, false>", "ilm::sphere_lights_kernel<1, false, false>"):
        v = bench.profiled_per_wave(k, "SQ_INSTS_VALU")
        assert v is not None and v["value"] > 1000


def test_contract_flags_and_defaults(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse_args()
    assert (a.gpus, a.steps, a.warmup) == (1, 200, 20)
    assert a.light_ms == 60.0 and a.light_frames >= 1 and a.cpu_seconds <= 30
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"])
    a = bench.parse_args()
    assert (a.gpus, a.steps, a.warmup) == (8, 20, 5)
    assert bench.PARTICLE_BYTES_PER_SLOT == 112 and bench.HBM_PEAK_GBS == 8000.0


def test_the_mesh_gbuffer_scene_is_what_the_row_says():
    """next_rows.gbuffer_2p5d_1080p: 256 height volumes (top + front faces) and 64 billboards as float32 vertex rows, 2 507 triangles with the
    ground plane's two."""
    import numpy as np
    gd, top, front, bb = bench.gbuffer_meshes_scene()
    assert top.dtype == np.float32 and front.dtype == np.float32 and bb.dtype == np.float32
    assert top.shape[1] == 9 and front.shape[1] == 9 and bb.shape == (256, 12)
    assert len(top) % 3 == 0 and len(front) % 3 == 0
    assert 2 + len(top) // 3 + len(front) // 3 + 128 == 2507
    assert gd.TwoPointFiveD != 0 and gd.DistanceFieldExtentZ == 128.0


def test_optional_rows_merge_and_the_watchdog_prints_the_fallback():
    """bench.run_optional_rows (N > 1): the optional frames are merged into scaling_detail's frames when they finish; when they do not, a
    watchdog THREAD has rank 0 print the record as it stood and ends the process with status 0 (the main thread may be stuck in a
    collective, so nothing may depend on it returning)."""
    import subprocess
    import sys
    import types
    calls = []
    frames = {"cfg3": {"composited_frame_ms": 1.0}}
    old = bench.exchange_variant_rows
    bench.exchange_variant_rows = lambda v: {"store_mode": {"composited_frame_ms": v.x}}
    try:
        bench.run_optional_rows([("cfg3", types.SimpleNamespace(x=0.5))], frames, 30, 0, lambda: calls.append("fallback"), lambda: calls.append("barrier"))
    finally:
        bench.exchange_variant_rows = old
    assert frames == {"cfg3": {"composited_frame_ms": 1.0, "store_mode": {"composited_frame_ms": 0.5}}} and calls == ["barrier"]
    code = ("import sys, time, types; sys.path.insert(0, %r); import bench\n"
            "bench.exchange_variant_rows = lambda v: time.sleep(1e6)\n"
            "bench.run_optional_rows([('cfg3', types.SimpleNamespace())], {'cfg3': {}}, 1, int(sys.argv[1]), lambda: print('FALLBACK', flush=True), lambda: None)\n"
            "print('NOT REACHED')\n") % ROOT
    for rank, want in ((0, "FALLBACK\n"), (1, "")):
        p = subprocess.run([sys.executable, "-c", code, str(rank)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout == want, (rank, p.stdout, p.stderr[-2000:])


def _row(value, ms, live=1000):
    blocks = [(ms * 1e-3 * 4, ms * 4 * 0.98)] * 3
    return bench.particle_row(1, live, 4, blocks, "stand-in kernel")


def test_the_one_gpu_headline_is_cfg4_whole_and_cfg2_stays_beside_it():
    """N = 1 (r06): `value`, `ms_per_step`, `roofline` and `config.workload` are the 64 M row (HBM-resident, the size the north star's particle
    target is quoted at); cfg2 (Infinity-Cache-resident) becomes `cfg2_cache_resident`.  Without the 64 M row (--no-cfg4-64m) cfg2 stays."""
    import copy
    c64 = _row(0, 1.25, live=67108864)
    c64["workload"] = "cfg4 whole on ONE GPU: 64 chunks of 1024^2 = 67108864 particles"
    roof = {"bound": "hbm", "achieved": 6400.0, "peak": bench.HBM_PEAK_GBS, "unit": "GB/s", "frac": 0.8, "traffic": None}
    out = {"metric": "m", "value": 55000.0, "unit": "Mparticle-steps/s", "n_gpus": 1, "steps": 4, "warmup": 0, "ms_per_step": 0.02, "config": {"workload": "cfg2: ...", "live_particles_per_step_avg": 1.1e6},
           "timed_blocks": {"blocks": 3}, "roofline": roof, "cfg4_full_64m_one_gpu": c64}
    rec = bench.finalize_record(copy.deepcopy(out), 1, False, 20.0)
    assert rec["value"] == c64["mparticle_steps_per_s"] and rec["ms_per_step"] == c64["ms_per_step"] and rec["roofline"] == c64["roofline"]
    assert rec["config"]["workload"].startswith("cfg4-64M on one GPU: 64 chunks of 1024^2") and rec["config"]["particles_per_gpu"] == 67108864
    assert rec["cfg2_cache_resident"]["mparticle_steps_per_s"] == 55000.0 and rec["cfg2_cache_resident"]["roofline"] == roof
    assert rec["summary"]["particles_cfg2"]["mparticle_steps_per_s"] == 55000.0 and rec["summary"]["particles_cfg4_64m_one_gpu"]["ms_per_step"] == c64["ms_per_step"]
    # the fraction is stated from both clocks: HIP events (the contract's) and ms_per_step
    assert 0 < rec["roofline"]["frac_from_ms_per_step"] <= rec["roofline"]["frac"]
    del out["cfg4_full_64m_one_gpu"]
    rec = bench.finalize_record(copy.deepcopy(out), 1, False, 20.0)
    assert rec["value"] == 55000.0 and "cfg2_cache_resident" not in rec and rec["config"]["workload"] == "cfg2: ..."


def test_the_n_gpu_headline_takes_the_live_count_row_when_it_was_measured():
    """N > 1 (r06): BASELINE config 4 is "per-chunk update + RCCL all-gather".  The rows with collectives run last under the watchdog; once
    measured, `value` is the step WITH ilm_group_live_counts and the communication-free figure stays as value_without_collectives; when they
    did not finish (or failed) the headline says that it has no collective."""
    import copy
    share, wl = _row(0, 0.20, live=8388608), _row(0, 0.21, live=8388608)
    wl["live_count_calls_per_block"] = 1.0
    roof = {"bound": "hbm", "achieved": 1.0, "peak": bench.HBM_PEAK_GBS, "unit": "GB/s", "frac": 0.1, "traffic": None}
    out = {"metric": "m", "value": 1.0, "unit": "Mparticle-steps/s", "n_gpus": 2, "steps": 4, "warmup": 0, "ms_per_step": 0.02, "config": {"workload": "cfg2: ..."},
           "timed_blocks": {"blocks": 3}, "roofline": roof, "cfg4_share_8m_particles": share}
    rec = bench.finalize_record(copy.deepcopy(out), 2, False, 20.0, {"with_live_counts": wl, "with_position_all_gather": {"error": "x"}})
    assert rec["value"] == wl["mparticle_steps_per_s"] < rec["value_without_collectives"] == share["mparticle_steps_per_s"]
    assert rec["ms_per_step"] == wl["ms_per_step"] and "ilm_group_live_counts" in rec["config"]["collective_in_the_timed_steps"]
    for rows in (None, {}, {"with_live_counts": {"error": "RuntimeError: x"}}):
        rec = bench.finalize_record(copy.deepcopy(out), 2, False, 20.0, rows)
        assert rec["value"] == share["mparticle_steps_per_s"] == rec["value_without_collectives"] and rec["config"]["collective_in_the_timed_steps"].startswith("none")
    sd = bench.scaling_detail(2, share, share, None, None, [1.0, 1.0], {}, collective_rows={"with_live_counts": wl, "with_position_all_gather": {"error": "x"}})
    assert sd["particles"]["with_live_counts"]["vs_without_collectives"] == round(wl["mparticle_steps_per_s"] / share["mparticle_steps_per_s"], 4)
    assert sd["particles"]["with_position_all_gather"] == {"error": "x"}


def test_the_collective_log_folds_repeats_and_keeps_the_order():
    log = bench.CollectiveLog()
    log.phase("a")
    for _ in range(3):
        log.add("ilm_group_host_all_gather", "ncclAllGather", 8)
    log.add("ilm_group_live_counts", "ncclAllGather", 32)
    log.phase("b")
    log.add("ilm_group_host_all_gather", "ncclAllGather", 8)
    t = log.table()
    assert len(t) == 4 and t[1].endswith("| x3") and "| a |" in t[1] and "ilm_group_live_counts" in t[2] and "| b |" in t[3] and t[3].endswith("| x1")


def test_the_particle_rows_with_collectives_run_first_under_the_watchdog():
    import types
    order = []
    old_p, old_x = bench.particle_collective_rows, bench.exchange_variant_rows
    bench.particle_collective_rows = lambda v: (order.append("particles"), {"with_live_counts": {"mparticle_steps_per_s": 1.0}})[1]
    bench.exchange_variant_rows = lambda v: (order.append("frames"), {"store_mode": {}})[1]
    rows, frames = {}, {"cfg3": {}}
    try:
        bench.run_optional_rows([("cfg3", types.SimpleNamespace())], frames, 30, 0, lambda: order.append("fallback"), lambda: order.append("barrier"),
                                particle_rows=(types.SimpleNamespace(), rows))
    finally:
        bench.particle_collective_rows, bench.exchange_variant_rows = old_p, old_x
    assert order == ["particles", "frames", "barrier"] and rows == {"with_live_counts": {"mparticle_steps_per_s": 1.0}} and "store_mode" in frames["cfg3"]


def test_a_plain_run_measures_the_headline_and_full_is_opt_in(monkeypatch):
    """Without --full a run is the headline alone; --full (implied by --dry-collectives) adds everything else; --dump-outputs belongs to
    the one-GPU headline, so it is refused where that row is not taken."""
    import pytest
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "3"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--dry-collectives"])
    assert bench.parse_args().full
    # N > 1 is the whole record: --full is implied, and the row switches keep their meaning there
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--no-cfg4-64m"])
    a = bench.parse_args()
    assert a.full and a.no_cfg4_64m
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cfg4", "--no-lighting", "--blocks", "3"])
    assert bench.parse_args().no_cfg4
    # one GPU without --full measures the headline alone: a switch that selects --full rows would be ignored, so it is refused
    for argv in (["--gpus", "2", "--dump-outputs", "out"], ["--full", "--no-cfg4-64m", "--dump-outputs", "out"], ["--steps", "0"],
                 ["--no-cfg4"], ["--no-cfg4-64m"], ["--no-lighting"], ["--no-next-rows"], ["--no-cpu-baseline"], ["--blocks", "3"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit):
            bench.parse_args()


def test_the_plain_line_carries_the_figures_a_full_record_leads_with():
    """headline_record (a run without --full) and finalize_record (--full, N = 1) put the same 64 M row in metric / value / unit /
    higher_is_better / dtype / ms_per_step / roofline; the plain line is a few hundred bytes."""
    import json
    import types
    c64 = _row(0, 1.25, live=67108864)
    c64["workload"] = "cfg4 whole on ONE GPU: 64 chunks of 1024^2 = 67108864 particles"
    rec = bench.headline_record(types.SimpleNamespace(steps=4, warmup=0), c64)
    out = {"metric": bench.METRIC, "value": 55000.0, "unit": "Mparticle-steps/s", "n_gpus": 1, "steps": 4, "warmup": 0, "ms_per_step": 0.02,
           "higher_is_better": True, "dtype": "f32", "config": {"workload": "cfg2: ..."}, "timed_blocks": {"blocks": 3},
           "roofline": {"bound": "hbm", "frac": 0.8}, "cfg4_full_64m_one_gpu": c64}
    full = bench.finalize_record(out, 1, False, 20.0)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "timed_blocks"):
        assert rec[k] == full[k], k
    assert rec["config"]["workload"] == full["config"]["workload"] and rec["steps"] == 4
    assert rec["value"] == c64["mparticle_steps_per_s"] and rec["unit"] == "Mparticle-steps/s" and rec["dtype"] == "f32"
    assert len(json.dumps(rec)) < 4096
    # one timed block is not called a median
    assert c64["timed_blocks"]["headline"] == "median block" and bench.particle_row(1, 10, 4, [(1e-3, 1.0)], "k")["timed_blocks"]["headline"] == "the one block"


class _StandInSystem:
    """ParticleSystem.Readback(chunk, plane) of `n_chunks` chunks of `m` slots whose values name chunk, slot, plane and component."""

    def __init__(self, n_chunks, m):
        import numpy as np
        self.Chunks, self.m, self.np = [None] * n_chunks, m, np

    def Readback(self, chunk, plane):
        np = self.np
        return (np.arange(self.m, dtype=np.float32)[:, None] * 8 + np.arange(4, dtype=np.float32) + plane * 0.25 + chunk * 1e6).astype(np.float32)


def test_the_output_dump_is_a_fixed_sample_of_the_planes_the_step_writes(tmp_path):
    import numpy as np
    from illuminant_amd import abi
    ps = _StandInSystem(3, 3 * bench.DUMP_SLOTS_PER_CHUNK)
    bench.dump_particle_outputs(ps, abi, 3, str(tmp_path / "a"))
    bench.dump_particle_outputs(ps, abi, 3, str(tmp_path / "b"))
    names = ("position", "velocity", "render_color", "render_data")
    slot = np.load(str(tmp_path / "a" / "particles_slot.npy"))
    assert slot.dtype == np.float64 and slot.shape == (3 * bench.DUMP_SLOTS_PER_CHUNK,) and len(np.unique(slot)) == len(slot)
    chunk, idx = (slot // ps.m).astype(np.int64), (slot % ps.m).astype(np.int64)
    assert list(np.bincount(chunk)) == [bench.DUMP_SLOTS_PER_CHUNK] * 3
    for name, plane in zip(names, (abi.PLANE_POSITION, abi.PLANE_VELOCITY, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA)):
        a = np.load(str(tmp_path / "a" / ("particles_%s.npy" % name)))
        assert a.dtype == np.float32 and a.shape == (len(slot), 4)
        want = np.stack([ps.Readback(c, plane)[i] for c, i in zip(chunk, idx)])
        assert np.array_equal(a, want), name
        assert np.array_equal(a, np.load(str(tmp_path / "b" / ("particles_%s.npy" % name)))), "the sample must not change from run to run"
    # the headline's 64 chunks stay within the 64 MB the option may write
    assert 64 * bench.DUMP_SLOTS_PER_CHUNK * (4 * 4 * 4 + 8) <= 64 << 20
