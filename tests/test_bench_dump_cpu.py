"""`bench.py --dump-outputs DIR`: the host side of the dump (no GPU) — the step's result dict cut to its live rows, stored
as float32 / float64, and a whole that stays under the size limit with a fixed row sample."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_step(hops=2, K=4, cap=16, C=3):
    """A GraphedTrainer result dict as the captured step leaves it: fixed-capacity buffers, live counts in 1-element tensors,
    garbage beyond them."""
    from grapes_amd.modules.gcn import GCN
    g = torch.Generator().manual_seed(0)
    out = dict(loss_c=torch.tensor(1.5), loss_gfn=torch.tensor(0.25), log_z=torch.tensor(-0.5), tot_log_prob=torch.tensor(-3.0),
               hop_stats=torch.randn(hops, 6, generator=g), n_all=torch.tensor([7], dtype=torch.int32),
               all_nodes=torch.arange(cap, dtype=torch.int32) * 3, logits=torch.randn(cap, C, generator=g),
               kept=[torch.arange(K, dtype=torch.int32) + 100 * h for h in range(hops)],
               kept_counts=[torch.tensor([K - h], dtype=torch.int32) for h in range(hops)],
               hop_logits=[torch.randn(cap, 1, generator=g) for _ in range(hops)],
               nb_local=[torch.tensor([5, 2, 9] + [10 ** 6] * (cap - 3), dtype=torch.int32) for _ in range(hops)],
               sizes=[torch.tensor([3], dtype=torch.int32) for _ in range(hops)])
    torch.manual_seed(0)
    return out, (GCN(5, [8, C]), GCN(5 + hops + 1, [8, 1]), GCN(5, [8, 1]))


def test_step_outputs_are_the_live_rows_in_float32_or_float64():
    sys.path.insert(0, ROOT)
    import bench
    out, models = _fake_step()
    d = bench.step_outputs(out, models)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["all_nodes"], np.arange(7) * 3.0) and d["all_nodes"].dtype == np.float64
    assert np.array_equal(d["logits"], out["logits"][:7].numpy()) and d["logits"].dtype == np.float32
    assert np.array_equal(d["kept_hop0"], [0, 1, 2, 3]) and np.array_equal(d["kept_hop1"], [100, 101, 102])
    for h in range(2):    # the candidates' logits, read through nb_local (the ids beyond the live count are never followed)
        assert np.array_equal(d[f"sampler_logits_hop{h}"], out["hop_logits"][h].view(-1)[[5, 2, 9]].numpy())
    assert float(d["loss_c"]) == 1.5 and d["hop_stats"].shape == (2, 6)
    for net, m in zip(("classifier", "sampler", "log_z_net"), models):
        sd = m.state_dict()
        assert sd and all(np.array_equal(d[f"{net}.{k}"], v.numpy()) for k, v in sd.items())


def test_random_sampling_step_has_no_gflownet_outputs():
    sys.path.insert(0, ROOT)
    import bench
    out, models = _fake_step()
    out.update(loss_gfn=None, log_z=None, hop_logits=[])
    d = bench.step_outputs(out, models)
    assert "loss_gfn" not in d and "log_z" not in d and not any(k.startswith("sampler_logits") for k in d)


def test_write_outputs_keeps_the_whole_under_the_limit_with_a_fixed_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    arrays = {"big": rng.standard_normal((4096, 64)).astype(np.float32), "small": np.arange(10, dtype=np.float64)}
    limit = 256 << 10
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), arrays, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    big = np.load(tmp_path / "a" / "big.npy")
    assert 0 < big.shape[0] < 4096 and big.shape[1] == 64
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))             # the same rows every run
    rows = [int(np.flatnonzero((arrays["big"] == r).all(1))[0]) for r in big]
    assert rows == sorted(rows)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])
    # under the limit: everything as it is
    bench.write_outputs(str(tmp_path / "c"), arrays)
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), arrays["big"])
