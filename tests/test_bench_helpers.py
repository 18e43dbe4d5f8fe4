"""bench.py's host-side helpers that never touch the GPU: CPU accounting of the baseline leg and the NUMA placement of a rank (CPU-only tests)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # (__name__ != "__main__": no argument parsing, no launch)
    return mod


def test_cpulist_parsing():
    b = _bench()
    assert b._cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    assert b._cpulist("") == [] and b._cpulist("5") == [5]


def test_usable_cpus_is_bounded_by_the_affinity_mask_and_the_quota():
    """the all-threads CPU leg must be sized by what this process may run on (affinity mask, cgroup quota), not by the machine's hardware threads."""
    b = _bench()
    u = b.usable_cpus()
    aff = len(os.sched_getaffinity(0))
    assert u["affinity_cpus"] == aff and 1 <= u["threads"] <= aff
    if u["cgroup_cpu_quota"] is not None:
        assert u["threads"] <= max(1, int(u["cgroup_cpu_quota"] + 1e-9))
    if u["physical_cores_in_mask"] is not None:
        assert 1 <= u["physical_cores_in_mask"] <= aff
    keep = os.sched_getaffinity(0)
    try:  # a narrower mask narrows the leg
        one = {sorted(keep)[0]}
        os.sched_setaffinity(0, one)
        assert b.usable_cpus()["threads"] == 1
    finally:
        os.sched_setaffinity(0, keep)


def test_rank_pinning_without_a_gpu_topology_changes_nothing():
    """No KFD topology in this container: the placement hint reports why it did nothing and leaves the mask alone (it must never cost a run)."""
    b = _bench()
    keep = os.sched_getaffinity(0)
    info = b.pin_rank_to_its_gpus_cores(0, 1)
    try:
        assert "pinned" in info and info["cpus_before"] == len(keep)
        if not os.path.isdir("/sys/class/kfd/kfd/topology/nodes"):
            assert info["pinned"] is False and "note" in info and os.sched_getaffinity(0) == keep
        else:
            assert (not info["pinned"]) or 1 <= info["cpus"] <= len(keep)
    finally:
        os.sched_setaffinity(0, keep)


def test_survey_bytes_table_matches_the_workloads():
    b = _bench()
    for key, wl in b.WORKLOADS.items():
        d = "f64" if str(wl["dtype"]).endswith("float64") else "f32"
        assert (key, d) in b.SURVEY_8D_BYTES, key


def test_dump_outputs_is_capped_seeded_and_float(tmp_path, monkeypatch):
    """--dump-outputs: every non-empty array of the returned Data as float32 / float64 .npy, the same environments in every array, the same
    sample from call to call, and under the size cap (checked here on the CPU Data of the ant workload with a cap small enough to force a sample)."""
    import numpy as np
    import torch

    b = _bench()
    wl = b.WORKLOADS["ant"]
    lite = b.mt.mjcf.from_xml_path(b.mt.test_data_path(wl["xml"] + ".xml"))
    mx = b.mt.device_put(lite, dtype=torch.float32)
    B = 64
    d = b.build_inputs(mx, B, torch.float32, "cpu")
    whole = b.dump_outputs(d, str(tmp_path / "whole"), B)
    assert whole["envs"] == B and whole["sample_seed"] is None
    arrays = b.data_arrays(d)
    names = sorted(n for n, t in arrays.items() if t.numel() > 0)
    assert sorted(f[:-4] for f in os.listdir(tmp_path / "whole")) == names and "contact_dist" in names
    assert arrays["act"].numel() == 0 and "act" not in names  # the ant has no actuator activations: nothing to write
    qvel = np.load(tmp_path / "whole" / "qvel.npy")
    assert qvel.dtype == np.float32 and np.array_equal(qvel, d.qvel.numpy())
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", whole["bytes"] // 4)
    runs = [b.dump_outputs(d, str(tmp_path / f"s{i}"), B) for i in range(2)]
    assert 0 < runs[0]["envs"] < B and runs[0]["bytes"] <= b.DUMP_CAP_BYTES and runs[0]["sample_seed"] is not None
    for n in names:
        x, y = (np.load(tmp_path / f"s{i}" / f"{n}.npy") for i in range(2))
        assert x.size > 0 and x.dtype in (np.float32, np.float64) and np.array_equal(x, y) and x.shape[0] == runs[0]["envs"], n
    idx = np.sort(np.random.RandomState(b.DUMP_SAMPLE_SEED).choice(B, runs[0]["envs"], replace=False))
    assert np.array_equal(np.load(tmp_path / "s0" / "qvel.npy"), qvel[idx])
