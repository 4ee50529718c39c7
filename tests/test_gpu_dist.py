"""Multi-GPU path on the one-GPU test box.

What CAN run here and does:
  * c2d_dist with the real RCCL transport and a world of one rank (dlopen of librccl.so.1, ncclGetUniqueId,
    ncclCommInitRank, ncclAllReduce / ncclBroadcast on device words, the id-file exchange);
  * the N > 1 host logic of the C++ drivers and of bench.py with two ranks that SHARE device 0 and sum their
    counters through the rehearsal build of the library (lib-rehearsal/libc2d.so, put in front of the product
    library with LD_LIBRARY_PATH / C2D_LIBRARY: a sum through small files) — RCCL itself refuses two ranks on
    one device ("Duplicate GPU detected"), so two-rank RCCL needs the multi-GPU node the round-end driver uses.
    The product library has no such transport (checked below).
The property under test everywhere: shards + one sum reproduce the single-process result exactly (random streams
are keyed by scene id and sample index)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd", "bin")
GEN = os.path.join(BIN, "generate_dataset")
CCP = os.path.join(BIN, "compute_collision_probability")
LIB = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd", "lib", "libc2d.so")
REH_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd", "lib-rehearsal")
REH_LIB = os.path.join(REH_DIR, "libc2d.so")
# the drivers find libc2d.so through their RUNPATH, which LD_LIBRARY_PATH precedes
REHEARSAL = {"LD_LIBRARY_PATH": REH_DIR + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""), "C2D_SHARE_DEVICE": "1"}


def run(cmd, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e, **kw)


def summary_of(out):
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout + out.stderr          # ONE aggregated line, from rank 0
    return json.loads(lines[0])


def test_c2d_dist_rccl_single_rank(eng, pkg, tmp_path):
    """The product transport end to end with a world of one: id by bytes and id by file."""
    d = eng.dist_init(0, 1, eng.dist_unique_id())
    assert d.transport == "rccl" and d.rank == 0 and d.world_size == 1
    buf = eng.to_device(np.array([5, 2**40 + 7, 0], np.uint64))
    d.all_reduce_sum_u64(buf, 3)
    d.broadcast_u64(buf, 3, root=0)
    d.barrier()
    d.all_reduce_sum_u64(buf, 3)
    d.synchronize()                     # the watched wait for queued collectives
    assert not d.timed_out
    assert buf.get().tolist() == [5, 2**40 + 7, 0]
    d.close()
    path = str(tmp_path / "id")
    d2 = eng.dist_init_file(0, 1, path, 30.0)
    assert d2.transport == "rccl" and not os.path.exists(path)   # the id file is removed once everyone joined
    d2.all_reduce_sum_u64(buf, 3)
    eng.synchronize()
    assert buf.get().tolist() == [5, 2**40 + 7, 0]
    d2.close()
    buf.free()
    with pytest.raises(pkg.C2DError):
        eng.dist_init(1, 1, eng.dist_unique_id())               # rank out of range


def test_generate_dataset_two_ranks_equal_one_rank(tmp_path):
    args = ["-n", "5", "-b", "900", "-s", "2", "--num_poses", "200", "--num_variances", "100", "--max_samples", "3000", "--seed", "77",
            "--spread", "3.5"]
    one = run([GEN, "--data_dir", str(tmp_path / "one")] + args)
    assert one.returncode == 0, one.stderr
    two = run([GEN, "--data_dir", str(tmp_path / "two"), "--gpus", "2"] + args, env=REHEARSAL)
    assert two.returncode == 0, two.stderr + two.stdout
    s1, s2 = summary_of(one), summary_of(two)
    assert s2["world_size"] == 2 and s2["aggregated_over_ranks"] == 2 and "file" in s2["reduce"]
    for key in ("batches", "scenes", "mc_samples", "hits", "cp_hist"):
        assert s1[key] == s2[key], key
    names = sorted(p.name for p in (tmp_path / "one").glob("[0-9]*.npy"))
    assert names == [f"{k}.npy" for k in range(2, 7)]
    for nme in names + ["poses.npy", "variances.npy"]:
        assert np.array_equal(np.load(tmp_path / "one" / nme).view(np.uint32), np.load(tmp_path / "two" / nme).view(np.uint32)), nme


def test_generate_dataset_default_seed_is_resolved_once(tmp_path):
    """Without --seed the launcher picks the time-based seed and hands the same one to every rank."""
    out = run([GEN, "--data_dir", str(tmp_path / "d"), "--gpus", "2", "-n", "2", "-b", "300", "--num_poses", "50", "--num_variances", "50",
               "--max_samples", "2000"], env=REHEARSAL)
    assert out.returncode == 0, out.stderr
    seeds = [ln for ln in out.stdout.splitlines() if ln.startswith("seed:")]
    assert len(seeds) == 1                                      # rank 0 narrates; one seed
    # hand-launched ranks without a seed and without a link must refuse instead of diverging
    bad = run([GEN, "--data_dir", str(tmp_path / "e"), "--rank", "0", "--world_size", "2", "-n", "2", "-b", "300"])
    assert bad.returncode != 0 and "--seed" in bad.stderr


def _ccp_inputs(tmp_path, wl, n_batches=5, N=500):
    din, dout = tmp_path / "in", tmp_path / "out"
    din.mkdir()
    poses, sds, var = wl.random_tables(50, 40, seed=3)
    rng = np.random.default_rng(1)
    for k in range(n_batches):
        s = np.empty((N, 4), np.float32)
        s[:, 0] = rng.uniform(-6, 6, N)
        s[:, 1] = rng.uniform(-6, 6, N)
        s[:, 2] = rng.integers(0, 40, N)
        s[:, 3] = rng.integers(0, 50, N)
        np.save(din / f"{k}.npy", s)

    def fresh_out(name):
        d = tmp_path / name
        (d / "meta").mkdir(parents=True)
        np.save(d / "poses.npy", poses.view(np.float32).reshape(-1, 3))
        np.save(d / "variances.npy", var)
        np.save(d / "meta" / "accuracy_bins.npy", np.array([0, .01, .1, 1], np.float32))
        np.save(d / "meta" / "bin_accuracy.npy", np.array([1e-4, 1e-3, 1e-2], np.float32))
        np.save(d / "0.npy", np.zeros((3, 5), np.float32))       # an existing batch: numbering continues at 1
        return d

    return din, fresh_out


def test_ccp_two_ranks_equal_one_rank_both_launch_styles(tmp_path, wl):
    din, fresh_out = _ccp_inputs(tmp_path, wl)
    common = ["--data_in", str(din), "--max_samples", "4000", "--seed", "9"]
    d1 = fresh_out("one")
    one = run([CCP, "--data_out", str(d1)] + common)
    assert one.returncode == 0, one.stderr
    s1 = summary_of(one)
    # (a) the driver launches its own ranks
    d2 = fresh_out("two")
    two = run([CCP, "--data_out", str(d2), "--gpus", "2"] + common, env=REHEARSAL)
    assert two.returncode == 0, two.stderr + two.stdout
    # (b) two processes started by hand (as a launcher would), id file given, NO --start_batch_count: rank 0's count is
    # broadcast, so the late starter cannot mis-number its files (racy start_batch_count)
    d3 = fresh_out("three")
    env = dict(os.environ, WORLD_SIZE="2", LOCAL_RANK="0", C2D_DIST_ID_FILE=str(tmp_path / "idfile"), LD_LIBRARY_PATH=REHEARSAL["LD_LIBRARY_PATH"])
    p0 = subprocess.Popen([CCP, "--data_out", str(d3)] + common, env=dict(env, RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    p1 = subprocess.Popen([CCP, "--data_out", str(d3)] + common, env=dict(env, RANK="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    o0, e0 = p0.communicate(timeout=600)
    o1, e1 = p1.communicate(timeout=600)
    assert p0.returncode == 0 and p1.returncode == 0, e0 + e1
    assert not [ln for ln in o1.splitlines() if ln.startswith("{")]            # only rank 0 prints the summary
    s3 = json.loads([ln for ln in o0.splitlines() if ln.startswith("{")][-1])
    s2 = summary_of(two)
    for s in (s2, s3):
        assert s["aggregated_over_ranks"] == 2
        for key in ("batches", "scenes", "mc_samples", "hits", "cp_hist"):
            assert s1[key] == s[key], key
    for d in (d2, d3):
        assert sorted(p.name for p in d.glob("[0-9]*.npy")) == [f"{k}.npy" for k in range(0, 6)]
        for k in range(1, 6):
            assert np.array_equal(np.load(d1 / f"{k}.npy").view(np.uint32), np.load(d / f"{k}.npy").view(np.uint32)), k
    # hand-launched ranks with neither a link nor --start_batch_count refuse
    bad = run([CCP, "--data_out", str(d3), "--rank", "1", "--world_size", "2"] + common)
    assert bad.returncode != 0 and "--start_batch_count" in bad.stderr


def test_ccp_single_pair_mode_sharded_equals_oracle(oracle, wl):
    """BASELINE config 3 through the driver: S samples of one scene split over ranks by sample index, one sum."""
    sc = wl.MC_PAIR_SCENE
    S = 3_000_001
    ref = oracle.mc_pair(sc["robot_w"], sc["robot_h"], sc["pos"], sc["pose"], sc["std_dev"], 1234, 0, 0, S)
    one = run([CCP, "--pair_samples", str(S), "--seed", "1234"])
    assert one.returncode == 0, one.stderr
    s1 = summary_of(one)
    two = run([CCP, "--pair_samples", str(S), "--seed", "1234", "--gpus", "2"], env=REHEARSAL)
    assert two.returncode == 0, two.stderr
    s2 = summary_of(two)
    assert s1["hits"] == ref == s2["hits"] and s1["samples"] == S == s2["samples"]
    assert s2["aggregated_over_ranks"] == 2 and abs(s2["p"] - ref / S) < 1e-9
    # the product transport with one rank: --dist_id_file makes a world of one go through RCCL
    rc = run([CCP, "--pair_samples", "100000", "--seed", "5", "--dist_id_file", "/tmp/c2d_test_id_%d" % os.getpid()])
    assert rc.returncode == 0, rc.stderr
    assert summary_of(rc)["reduce"] == "rccl"


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus N` without a launcher (how the round-end driver calls it): rehearsed with two ranks
    sharing the device (gloo rendezvous + file transport), and with one rank through the real RCCL reduce."""
    small = ["--steps", "3", "--warmup", "1", "--pairs", "1000000", "--mc-samples", "1000000", "--mc-reps", "1", "--scenes", "20000",
             "--scenes-max-samples", "3000", "--poly-pairs", "200000", "--poly-reps", "2", "--poly-scenes", "20000", "--no-cpu-baseline", "--prewarm-ms", "5", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device", "--backend", "gloo"] + small,
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["ranks_in_reduce"] == 2 and "c2d_dist" in j["config"]["reduce"] and "rehearsal" in j["config"]["reduce"]
    assert abs(j["mc"]["probability"] - 0.5537) < 5e-3 and j["poly"]["collide_rate"] > 0.03
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist"] + small, capture_output=True, text=True, timeout=900,
                         env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads(out.stdout.strip().splitlines()[-1])
    assert j["n_gpus"] == 1 and "rccl" in j["config"]["reduce"]
    # a failing rank must fail the launcher
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device", "--backend", "gloo", "--pairs", "-5"] + small[6:],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and not out.stdout.strip()


def test_bench_with_four_ranks_sharing_the_device(tmp_path):
    """The round-end driver runs `bench.py --gpus 8` on a box this build never sees.  The pool lets at most six processes hold one
    card open — the test runner is one, torch's launcher another — so the largest rehearsal INSIDE the suite is four ranks sharing
    the device (gloo rendezvous, the file transport of the rehearsal build; profiles/r05_rehearse.sh runs five and six outside it):
    one JSON line, four ranks in the reduce, and the sharding identities of DESIGN.md §7 — the ranks' Monte-Carlo sample ranges
    and scene ranges are exactly the one-rank run over N times the range, so probabilities and totals are EQUAL."""
    N = 4
    small = ["--steps", "3", "--warmup", "1", "--pairs", "400000", "--mc-reps", "1", "--scenes-max-samples", "3000", "--poly-pairs", "100000",
             "--poly-reps", "2", "--poly-scenes", "0", "--no-cpu-baseline", "--prewarm-ms", "5", "--no-pose", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(N), "--share-device", "--backend", "gloo",
                          "--mc-samples", "1000000", "--scenes", "10000"] + small, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == N and j["config"]["ranks_in_reduce"] == N and "rehearsal" in j["config"]["reduce"]
    assert j["config"]["rccl_version"] == 0 and j["config"]["rccl_library"] == "file (rehearsal)" and j["config"]["torch_backend"] == "gloo"
    for r in range(N):  # every rank said which card it sits on
        assert f"[bench] rank {r} of {N}: device 0" in out.stderr, out.stderr[-3000:]
    # what makes the N > 1 line readable: every rank's own kernel time, the closing reduce by itself, and the rate of
    # the kernels alone beside `value`, in every leg that closes with the reduce
    spreads = [j["roofline"]["kernel_ms_ranks"], j["mc"]["kernel_ms_ranks"], j["scenes"]["device_loop_ms_ranks"],
               j["scenes"]["fixed_samples"]["device_loop_ms_ranks"], j["poly"]["roofline"]["kernel_ms_ranks"],
               j["poly"]["binned"]["roofline"]["kernel_ms_ranks"]]
    for sp in spreads:
        assert sp["ranks"] == N and sp["max"] >= sp["median"] >= sp["min"] > 0 and 0 <= sp["slowest_rank"] < N, sp
    for leg in (j, j["mc"], j["scenes"], j["poly"], j["poly"]["binned"]):
        assert leg["value_kernels_only"] > 0, leg.get("metric")
        ru = leg["reduce_us"]
        assert ru["reps"] > 0 and ru["event_max"] >= ru["event_median"] >= ru["event_min"] >= 0 and ru["host_median"] > 0, ru
    assert j["scenes"]["fixed_samples"]["value_kernels_only"] > 0
    # the kernels alone are never slower than the region that contains them, and the region's remainder is stated
    assert j["value_kernels_only"] >= j["value"] * 0.999
    sd = j["scaling_detail"]
    assert sd["barrier_us"] > 0 and abs(sd["timed_region_ms"] - j["ms_per_step"] * j["steps"]) < 1e-3
    assert abs(sd["timed_region_minus_kernels_us"] - (sd["timed_region_ms"] - sd["kernels_ms_slowest_rank"]) * 1e3) < 1.0
    for rf in (j["roofline"], j["poly"]["roofline"], j["poly"]["binned"]["roofline"]):
        assert 0 < rf["frac_slowest_rank"] <= rf["frac"] * 1.0001, rf
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mc-samples", str(N * 1000000), "--scenes", str(N * 10000)] + small,
                         capture_output=True, text=True, timeout=900, env=env)
    assert one.returncode == 0, one.stderr[-3000:]
    j1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert j1["n_gpus"] == 1 and j1["config"]["ranks_in_reduce"] == 1
    assert j["mc"]["probability"] == j1["mc"]["probability"]                               # hits over [0, N S) either way
    assert j["scenes"]["pooled_hit_fraction"] == j1["scenes"]["pooled_hit_fraction"]       # scene ids [0, N n) either way
    assert j["scenes"]["mean_samples_per_point"] == j1["scenes"]["mean_samples_per_point"]
    assert j["scenes"]["fixed_samples"]["pooled_hit_fraction"] == j1["scenes"]["fixed_samples"]["pooled_hit_fraction"]


def test_c2d_dist_error_paths(eng, pkg, tmp_path):
    """A rank that never finds its peers gets C2D_ERR_DIST within the timeout instead of hanging; bad arguments are refused."""
    import time

    t0 = time.time()
    with pytest.raises(pkg.C2DError) as ei:
        eng.dist_init_file(1, 2, str(tmp_path / "never_written"), 1.0)     # rank 0 never writes the id
    assert ei.value.status == -6 and time.time() - t0 < 10 and "id file" in str(ei.value)
    with pytest.raises(pkg.C2DError):
        eng.dist_init_file(0, 0, str(tmp_path / "x"), 1.0)
    with pytest.raises(ValueError):
        eng.dist_init(0, 1, b"short")
    # the product library has one transport and no environment variable changes that
    os.environ["C2D_DIST_TRANSPORT"] = "file"
    try:
        d = eng.dist_init(0, 1, eng.dist_unique_id())
    finally:
        del os.environ["C2D_DIST_TRANSPORT"]
    assert d.transport == "rccl"
    d.close()


def test_watchdog_times_out_instead_of_hanging(eng, pkg):
    """A communicator whose second rank never arrives: ncclCommInitRank would block for ever; the watchdog returns
    C2D_ERR_DIST after $C2D_DIST_TIMEOUT_S.  Run in a child process, because the helper thread stays inside RCCL."""
    code = (
        "import os, sys, time; sys.path.insert(0, %r)\n"
        "os.environ['C2D_DIST_TIMEOUT_S'] = '4'\n"
        "from __graft_entry__ import load_package; pkg = load_package(); eng = pkg.Engine(0)\n"
        "t0 = time.time()\n"
        "try:\n"
        "    eng.dist_init(0, 2, eng.dist_unique_id())\n"
        "    print('NO ERROR')\n"
        "except pkg.C2DError as e:\n"
        "    print('STATUS', e.status, round(time.time() - t0, 1), str(e))\n"
        "sys.stdout.flush(); os._exit(0)\n" % ROOT)
    out = run([sys.executable, "-c", code])
    assert "STATUS -6" in out.stdout and "did not complete within 4 s" in out.stdout, out.stdout + out.stderr


def test_driver_ends_at_once_when_a_peer_never_arrives(tmp_path):
    """a driver whose peer never shows up must report C2D_ERR_DIST and END — not return through exit(), whose HIP
    teardown would race the helper thread the watchdog left inside RCCL.  Product library, real RCCL: rank 0 of a world of two,
    rank 1 never started, $C2D_DIST_TIMEOUT_S = 4 (the drivers pass 0 = "the default" to c2d_dist_init_file, so the variable
    applies to them).  Both modes of the driver that open a link."""
    import time

    env = {"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "C2D_DIST_TIMEOUT_S": "4"}
    for k, extra in enumerate((["--pair_samples", "100000", "--seed", "1"], None)):
        e = dict(env, C2D_DIST_ID_FILE=str(tmp_path / f"id{k}"))
        if extra is None:  # dataset mode needs its directories to exist before it opens the link
            (tmp_path / "in").mkdir()
            (tmp_path / "out" / "meta").mkdir(parents=True)
            np.save(tmp_path / "in" / "0.npy", np.zeros((4, 4), np.float32))
            np.save(tmp_path / "out" / "poses.npy", np.ones((2, 3), np.float32))
            np.save(tmp_path / "out" / "variances.npy", np.ones((2, 5), np.float32) * 0.1)
            np.save(tmp_path / "out" / "meta" / "accuracy_bins.npy", np.array([0, .01, .1, 1], np.float32))
            np.save(tmp_path / "out" / "meta" / "bin_accuracy.npy", np.array([1e-4, 1e-3, 1e-2], np.float32))
            extra = ["--data_in", str(tmp_path / "in"), "--data_out", str(tmp_path / "out"), "--seed", "2"]
        t0 = time.time()
        out = subprocess.run([CCP] + extra, capture_output=True, text=True, timeout=120, env=dict(os.environ, **e))
        took = time.time() - t0
        assert out.returncode != 0, out.stdout + out.stderr
        assert "did not complete within 4 s" in out.stderr, out.stderr
        assert took < 60, took   # the 4-second limit plus start-up, not the 300-second default, and no hang in the teardown


def test_peer_that_dies_after_the_link_was_built(tmp_path, pkg):
    """c2d_dist_stream_synchronize / the drivers' DistLink::sum: the result collectives are under the deadline too.  Rehearsed with
    the file transport: rank 1 joins the link and then dies before the reduce; rank 0 must fail within its limit."""
    import time

    code = (
        "import os, sys, time; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from __graft_entry__ import load_package; pkg = load_package(); eng = pkg.Engine(0, lib_path=%r)\n"
        "rank = int(sys.argv[1])\n"
        "d = eng.dist_init_file(rank, 2, sys.argv[2], 3.0)\n"
        "if rank == 1: os._exit(0)\n"
        "buf = eng.to_device(np.array([1], np.uint64)); t0 = time.time()\n"
        "try:\n"
        "    d.all_reduce_sum_u64(buf, 1); d.synchronize(); print('NO ERROR')\n"
        "except pkg.C2DError as e:\n"
        "    print('STATUS', e.status, round(time.time() - t0, 1), str(e))\n"
        "sys.stdout.flush(); os._exit(0)\n" % (ROOT, REH_LIB))
    idf = str(tmp_path / "id")
    p0 = subprocess.Popen([sys.executable, "-c", code, "0", idf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    p1 = subprocess.Popen([sys.executable, "-c", code, "1", idf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    o0, e0 = p0.communicate(timeout=120)
    p1.communicate(timeout=120)
    assert "STATUS -6" in o0 and "timed out" in o0, o0 + e0


def test_rehearsal_transport_lives_in_its_own_build(eng, pkg):
    """The file transport exists only in lib-rehearsal/libc2d.so: the product library holds none of its strings, and the
    rehearsal build — same C-ABI — reports itself."""
    prod, reh = open(LIB, "rb").read(), open(REH_LIB, "rb").read()
    assert b"c2d-file-transport" not in prod and b"rehearsal" not in prod
    assert b"c2d-file-transport" in reh
    e2 = pkg.Engine(0, lib_path=REH_LIB)
    d = e2.dist_init(0, 1, e2.dist_unique_id())
    assert d.transport == "file (rehearsal)" and d.world_size == 1
    buf = e2.to_device(np.array([7, 9], np.uint64))
    d.all_reduce_sum_u64(buf, 2)
    d.broadcast_u64(buf, 2)
    d.barrier()
    assert buf.get().tolist() == [7, 9]
    d.close()
    buf.free()
    with pytest.raises(pkg.C2DError):
        e2.dist_init(0, 1, eng.dist_unique_id())   # an RCCL id is not a rehearsal id
    e2.close()


def _visible_gpus():
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=300)
    try:
        return int(out.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return 0


def test_rccl_with_two_real_ranks_when_two_gpus_are_visible(tmp_path):
    """The product path with N > 1: two ranks on two devices, ncclCommInitRank + ncclAllReduce over xGMI through libc2d — bench.py
    starting its own ranks and the drivers' --gpus 2.  Needs two GPUs: skipped on the one-GPU test box, runs wherever the suite is
    started on a multi-GPU node."""
    if _visible_gpus() < 2:
        pytest.skip("needs two visible GPUs (RCCL refuses two ranks on one device)")
    small = ["--steps", "3", "--warmup", "1", "--pairs", "1000000", "--mc-samples", "1000000", "--mc-reps", "1", "--scenes", "20000",
             "--scenes-max-samples", "3000", "--poly-pairs", "200000", "--poly-reps", "2", "--poly-scenes", "20000", "--no-cpu-baseline", "--prewarm-ms", "5", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + small, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads(out.stdout.strip().splitlines()[-1])
    assert j["n_gpus"] == 2 and j["config"]["ranks_in_reduce"] == 2 and "rccl" in j["config"]["reduce"]
    assert abs(j["mc"]["probability"] - 0.5537) < 5e-3
    args = ["-n", "4", "-b", "900", "--num_poses", "200", "--num_variances", "100", "--max_samples", "3000", "--seed", "77"]
    one = run([GEN, "--data_dir", str(tmp_path / "one")] + args)
    two = run([GEN, "--data_dir", str(tmp_path / "two"), "--gpus", "2"] + args)
    assert one.returncode == 0 and two.returncode == 0, one.stderr + two.stderr
    s1, s2 = summary_of(one), summary_of(two)
    assert s2["aggregated_over_ranks"] == 2 and s2["reduce"] == "rccl"
    for key in ("batches", "scenes", "mc_samples", "hits", "cp_hist"):
        assert s1[key] == s2[key], key
    for k in range(4):
        assert np.array_equal(np.load(tmp_path / "one" / f"{k}.npy").view(np.uint32), np.load(tmp_path / "two" / f"{k}.npy").view(np.uint32)), k
