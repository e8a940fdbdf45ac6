"""Multi-process (gloo, world_size 2, CPU) tests of the layer-sharded path: shard planning, every
weight owned exactly once, the rooted gather (and the scatter) of packed results reproduces the
single-process result bit-exactly, and bench.py's multi-rank record.  The GPU quantizer is replaced
by the oracle here (CPU box); on MI355X the same code runs the batched kernel and RCCL."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from iron_weight_only_quant_amd import shard


def test_plan_covers_every_weight_once():
    shapes = shard.model_linear_shapes("llama2-70b")
    assert len(shapes) == 560
    for world in (1, 2, 4, 8):
        bins = shard.plan_shards(shapes, world)
        flat = sorted(i for b in bins for i in b)
        assert flat == list(range(len(shapes)))
        assert shard.shard_imbalance(shapes, bins) < 1.02
    assert sum(r * c for _, (r, c) in shapes) == 68_451_041_280  # 560 Linear weights
    s7 = shard.model_linear_shapes("llama2-7b")
    assert len(s7) == 224 and sum(r * c for _, (r, c) in s7) == 6_476_005_376


def _oracle_quantize_fn(bits, group, sym):
    from oracle import iwq_oracle as O

    def fn(ws):
        codes, scales, zeros = [], [], []
        for w in ws:
            r = O.quantlinear_int(w.numpy(), w_bit=bits, w_group_size=group, symmetric=sym)
            w.copy_(torch.from_numpy(r.dequant))
            codes.append(torch.from_numpy(O.pack_codes(r.codes, bits).reshape(-1)))
            scales.append(torch.from_numpy(r.scales.reshape(-1)))
            zeros.append(None if r.zeros is None else torch.from_numpy(r.zeros.reshape(-1)))
        return codes, scales, zeros
    return fn


def _small_model():
    return [(f"layers.{i}.{n}", (r, c)) for i in range(3) for n, r, c in
            [("q", 64, 256), ("up", 160, 256), ("down", 64, 384)]]


def _worker(rank, world, port, out_q, sym):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle.synth import synth
        shapes = _small_model()
        bins = shard.plan_shards(shapes, world)
        mine = {shapes[i][0]: torch.from_numpy(synth(500 + i, shapes[i][1], "float16")) for i in bins[rank]}
        res = shard.quantize_shard(mine, 4, 128, sym, quantize_fn=_oracle_quantize_fn(4, 128, sym))
        names_per_rank = [[shapes[i][0] for i in b] for b in bins]
        got = shard.gather_to_rank0(res, dict(shapes), names_per_rank, 4, 128, sym)
        if rank == 0:
            out_q.put({k: (v[0].numpy(), v[1].numpy(), None if v[2] is None else v[2].numpy()) for k, v in got.items()})
    finally:
        dist.destroy_process_group()


def _subgroup_worker(rank, world, port, out_q, group):
    """World 3; the gather runs inside the sub-group of global ranks {1, 2} (its root is global rank
    1): point-to-point peers must be translated to global ranks."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pg = dist.new_group([1, 2])
        if rank in (1, 2):
            from oracle.synth import synth
            shapes = _small_model()
            bins = shard.plan_shards(shapes, 2)
            me = rank - 1
            mine = {shapes[i][0]: torch.from_numpy(synth(700 + i, shapes[i][1], "float16")) for i in bins[me]}
            res = shard.quantize_shard(mine, 4, group, False, quantize_fn=_oracle_quantize_fn(4, group, False))
            got = shard.gather_to_rank0(res, dict(shapes), [[shapes[i][0] for i in b] for b in bins], 4, group,
                                        False, pg=pg)
            if me == 0:
                out_q.put({k: (v[0].numpy(), v[1].numpy(), v[2].numpy()) for k, v in got.items()})
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("group", [128, -2])
def test_gloo_subgroup_gather_uses_global_peers(group):
    """gather_to_rank0 inside a sub-group that does not start at global rank 0, and with
    per-channel parameters (G = rows, not rows * cols / group)."""
    from oracle import iwq_oracle as O
    from oracle.synth import synth
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, 3, port, q, group)) for r in range(3)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shapes = _small_model()
    assert set(got) == {n for n, _ in shapes}
    for i, (n, shp) in enumerate(shapes):
        r = O.quantlinear_int(synth(700 + i, shp, "float16"), w_bit=4, w_group_size=group, symmetric=False)
        codes, scales, zeros = got[n]
        assert np.array_equal(codes, O.pack_codes(r.codes, 4).reshape(-1))
        assert np.array_equal(scales.view(np.uint16), r.scales.reshape(-1).view(np.uint16))
        assert np.array_equal(zeros.view(np.uint16), r.zeros.reshape(-1).view(np.uint16))
    assert shard.packed_nbytes((64, 256), 4, -2, False) == 64 * 128 + 64 * 4
    assert shard.packed_nbytes((64, 256), 4, -1, True) == 64 * 128 + 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("sym", [False, True])
def test_gloo_world2_gather_matches_single_process(sym):
    from oracle import iwq_oracle as O
    from oracle.synth import synth
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, sym)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shapes = _small_model()
    assert set(got) == {n for n, _ in shapes}
    for i, (n, shp) in enumerate(shapes):
        r = O.quantlinear_int(synth(500 + i, shp, "float16"), w_bit=4, w_group_size=128, symmetric=sym)
        codes, scales, zeros = got[n]
        assert np.array_equal(codes, O.pack_codes(r.codes, 4).reshape(-1))
        assert np.array_equal(scales.view(np.uint16), r.scales.reshape(-1).view(np.uint16))
        if not sym:
            assert np.array_equal(zeros.view(np.uint16), r.zeros.reshape(-1).view(np.uint16))


def _scatter_worker(rank, world, port, out_q):
    import torch.distributed as dist
    from iron_weight_only_quant_amd import shard
    from oracle.synth import synth
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shapes = _small_model()
        bins = shard.plan_shards(shapes, world)
        layouts = [shard.bin_layout(shapes, b) for b in bins]
        sends, recv = None, None
        if rank == 0:  # rank 0 holds the whole model, one flat buffer per destination rank
            sends = []
            for lay, tot in layouts:
                flat = torch.zeros(tot, dtype=torch.float16)
                for name, off, (r, c) in lay:
                    i = [n for n, _ in shapes].index(name)
                    flat[off: off + r * c] = torch.from_numpy(synth(500 + i, (r, c), "float16").reshape(-1))
                sends.append(flat)
        else:
            recv = torch.empty(layouts[rank][1], dtype=torch.float16)
        mine = shard.scatter_from_rank0(sends, recv)
        got = {k: v.numpy().copy() for k, v in shard.views_of(mine, layouts[rank][0]).items()}
        out_q.put((rank, got))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_scatter_from_rank0():
    """Every rank receives exactly its bin's weights, bit for bit, from rank 0."""
    from oracle.synth import synth
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_scatter_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shapes = _small_model()
    from iron_weight_only_quant_amd import shard
    bins = shard.plan_shards(shapes, 2)
    for r in range(2):
        assert set(res[r]) == {shapes[i][0] for i in bins[r]}
        for name, arr in res[r].items():
            i = [n for n, _ in shapes].index(name)
            assert np.array_equal(arr.view(np.uint16), synth(500 + i, shapes[i][1], "float16").view(np.uint16))


def test_bench_gpus2_spawns_ranks_and_rooted_gather_moves_each_byte_once():
    """`bench.py --gpus 2` (no WORLD_SIZE: the driver's command form) spawns two rank processes
    itself; over gloo on the CPU (--dry-run) the rooted gather delivers every tensor to rank 0 and
    moves exactly rank 1's packed bytes once (an all_gather would move them N times)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run", "--full",
                        "--model", "opt-125m"], capture_output=True, text=True, timeout=300, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints the only JSON line
    rec = json.loads(lines[0])
    assert rec["world"] == 2 and rec["tensors"] == 72 and rec["tensors_at_rank0"] == 72
    per_rank = rec["plan_packed_bytes_per_rank"]
    shapes = shard.model_linear_shapes("opt-125m")
    assert sum(per_rank) == sum(shard.packed_nbytes(s, 4, 128, False) for _, s in shapes)
    assert rec["gather_sent_bytes"] == per_rank[1] == rec["gather_recv_bytes"]
    # the N = 2 record is complete for the driver's scaling runs: ranks, devices, the roofline over
    # ranks (slowest rank's kernel time, every rank's fraction) and the CPU baseline on rank 0
    assert rec["ranks"] == 2 and "n_devices" in rec
    roof = rec["roofline"]
    assert roof["kernel_ms"] == 1.25 and roof["kernel_ms_basis"] == "max over ranks"
    assert [p["rank"] for p in roof["per_rank"]] == [0, 1]
    assert roof["per_rank"][0]["kernel_ms"] == 1.0 and roof["frac"] > 0
    # every rank's own copy ceiling and kernel / ceiling ratio; the top level is the lowest rank's
    assert [p["ceiling_GBps"] for p in roof["per_rank"]] == [5000.0, 4900.0]
    assert roof["ceiling"]["GBps"] == 4900.0
    assert roof["kernel_over_ceiling"] == min(p["kernel_over_ceiling"] for p in roof["per_rank"])
    # the north star's collectives are in the DEFAULT N = 2 record (timed apart from value): the rooted
    # gather of the packed results and the scatter of the model's fp16 bins from rank 0
    assert rec["gather_ms"] > 0 and rec["gather_bytes_to_rank0"] == per_rank[1] and rec["gather_GBps"] > 0
    lay = [shard.bin_layout(shapes, b)[1] for b in shard.plan_shards(shapes, 2)]
    assert rec["scatter_ms"] > 0 and rec["scatter_bytes_from_rank0"] == 2 * lay[1]
    assert rec["scatter_verified"] is True
    cpu = rec["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["kind"] == "port" and "OPT-125M" in cpu["sample"]


def test_bench_gpus8_dry_run_rehearses_the_eight_rank_path():
    """The driver's N = 8 command form (`bench.py --gpus 8`, no WORLD_SIZE) on the CPU over gloo: 8
    spawned ranks, 8 disjoint bins covering every weight, the rooted gather moving exactly the
    non-root bins' packed bytes once, the scatter delivering every rank its own bin (checked on each
    rank), and one per-rank roofline row with its own ceiling for each of the 8 ranks.  Its wall time is
    recorded (the driver allows the 8-GPU bench 600 s)."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "1"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-run", "--full",
                        "--model", "opt-125m"], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    shapes = shard.model_linear_shapes("opt-125m")
    bins = shard.plan_shards(shapes, 8)
    assert len(bins) == 8 and all(bins)
    assert sorted(i for b in bins for i in b) == list(range(len(shapes)))
    assert rec["world"] == 8 and rec["ranks"] == 8 and rec["tensors"] == 72 and rec["tensors_at_rank0"] == 72
    per_rank = rec["plan_packed_bytes_per_rank"]
    assert per_rank == [sum(shard.packed_nbytes(shapes[i][1], 4, 128, False) for i in b) for b in bins]
    assert rec["gather_bytes_to_rank0"] == sum(per_rank[1:]) == rec["gather_sent_bytes"] == rec["gather_recv_bytes"]
    assert rec["scatter_verified"] is True
    lay = [shard.bin_layout(shapes, b)[1] for b in bins]
    assert rec["scatter_bytes_from_rank0"] == 2 * sum(lay[1:])
    roof = rec["roofline"]
    assert [p["rank"] for p in roof["per_rank"]] == list(range(8))
    assert all(p["ceiling_GBps"] > 0 and p["kernel_over_ceiling"] > 0 for p in roof["per_rank"])
    assert roof["kernel_ms"] == 1.0 + 0.25 * 7 and roof["kernel_ms_basis"] == "max over ranks"
    print(f"[8-rank dry run] wall {wall:.1f} s (driver limit 600 s)")
    assert wall < 300


def test_bench_world_size_must_match_gpus():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run",
                        "--model", "opt-125m"], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode != 0 and "world size 1 != --gpus 2" in r.stderr
