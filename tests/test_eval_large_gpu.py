"""Full-batch evaluation over graphs with 2^31 or more CSR entries (grapes_amd/full_graph.py, csrc/spmm_large.hip): the
row-blocked, layer-by-layer pass with 64-bit row offsets — forced on small graphs against the CPU oracle, on circulant graphs
past the 2^31st entry against an exact fp64 reference, on papers100M at its real shape, and through the CLI."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import grapes_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _small(asymmetric, F, C, H, depth, seed=3):
    from grapes_amd import synth
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    n = 6000
    indptr, indices = synth.synth_csr_numpy(n, 14.0, 600, seed=seed)      # (the graphs of test_eval_gpu._setup: hub rows > 1024)
    rng = np.random.default_rng(seed + 1)
    if asymmetric:   # a third of the entries dropped (directed) + self-loops on every fifth node (PyG replaces them)
        rows = np.repeat(np.arange(n), np.diff(indptr))
        keep = rng.random(len(indices)) > 0.33
        ei = np.stack([np.concatenate([rows[keep], np.arange(0, n, 5)]), np.concatenate([indices[keep], np.arange(0, n, 5)])])
        indptr, indices = O.build_csr(ei, n)
    X = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, C, n))
    torch.manual_seed(seed)
    dims = [H] * (depth - 1) + [C]
    rc, rgf = O.GCNRef(F, dims), O.GCNRef(F + depth + 1, [H, 1])
    c, gf = GCN(F, dims).cuda(), GCN(F + depth + 1, [H, 1]).cuda()
    c.load_state_dict(rc.state_dict()); gf.load_state_dict(rgf.state_dict())
    return indptr, indices, X, y, rc, rgf, c, gf, DeviceGraph.from_csr(indptr, indices), rng


@pytest.mark.parametrize("F,C", [(100, 7), (128, 47)])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("asymmetric", [False, True])
def test_forced_large_path_matches_oracle(asymmetric, depth, F, C):
    _cuda()
    from grapes_amd import full_graph
    from grapes_amd.eval import evaluate
    n, H = 6000, 256 if depth == 3 else 64
    indptr, indices, X, y, rc, rgf, c, gf, g, rng = _small(asymmetric, F, C, H, depth)
    plan = g.full_graph_plan(hub_chunk=64)                  # (rows above 64 entries: hub rows cut into work items)
    assert int(np.diff(indptr).max()) > 2 * 64 and plan.item_cap >= 3
    nodes = np.sort(rng.permutation(n)[:1500])
    mask = torch.zeros(n, dtype=torch.bool); mask[torch.from_numpy(nodes)] = True
    data = types.SimpleNamespace(x=X, y=y)
    args = types.SimpleNamespace(sampling_hops=depth, num_samples=64, use_indicators=True, eval_block_rows=777)
    acc, f1, pred = evaluate(c, gf, data, args, g, mask=mask, full_batch=True, return_predictions=True, large_graph=True)
    oacc, of1, opred = O.evaluate(indptr, indices, X, y, nodes, rc, rgf, sampling_hops=depth, num_samples=64, full_batch=True)
    assert pred.shape == opred.shape
    flips = float((pred.cpu() != opred).float().mean())
    assert flips <= 2e-3, flips
    # metrics: those of the predictions returned (equal to the oracle's wherever no near-tie flipped)
    assert abs(acc - float((pred.cpu() == y[torch.from_numpy(nodes)]).float().mean())) < 1e-6 and acc == f1
    if flips == 0.0:
        assert abs(acc - oacc) < 1e-6 and abs(f1 - of1) < 1e-6
    # whole-graph logits through the module path (forced) and through a ragged row block, against the oracle's GCN
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    rl, _ = rc(X, torch.from_numpy(np.stack([rows, indices.astype(np.int64)])))
    rl = rl.detach()
    scale = max(1.0, float(rl.abs().max()))
    with torch.inference_mode():
        lm, _ = c(X.cuda(), g, large_graph=True)
        lb = full_graph.gcn_forward(c, X.cuda(), g, block_rows=777)
        lb2 = full_graph.gcn_forward(c, X.cuda(), g, block_rows=777)
    assert float((lm.cpu() - rl).abs().max()) <= 1e-5 * scale
    assert float((lb.cpu() - rl).abs().max()) <= 1e-5 * scale
    assert torch.equal(lb, lb2)                                                 # fixed summation order: bit-identical
    _, _, pred2 = evaluate(c, gf, data, args, g, mask=mask, full_batch=True, return_predictions=True, large_graph=True)
    assert torch.equal(pred, pred2)
    assert plan is g.full_graph_plan() and plan.symmetric == (not asymmetric)
    # the int32 path is untouched and still cached on its own
    assert g.gcn_prepared() is g.gcn_prepared()


def test_forced_large_path_multilabel_and_training_refusal():
    _cuda()
    from grapes_amd.eval import evaluate
    n, F, C, H = 6000, 64, 11, 128
    indptr, indices, X, _, rc, rgf, c, gf, g, rng = _small(True, F, C, H, 2, seed=5)
    assert g.full_graph_plan(hub_chunk=64).item_cap > 0
    ym = torch.from_numpy((rng.random((n, C)) < 0.3).astype(np.float32))
    nodes = np.sort(rng.permutation(n)[:1200])
    mask = torch.zeros(n, dtype=torch.bool); mask[torch.from_numpy(nodes)] = True
    data = types.SimpleNamespace(x=X, y=ym)
    args = types.SimpleNamespace(sampling_hops=2, num_samples=32, use_indicators=True, eval_block_rows=500)
    acc, f1, pred = evaluate(c, gf, data, args, g, mask=mask, full_batch=True, return_predictions=True, large_graph=True)
    oacc, of1, opred = O.evaluate(indptr, indices, X, ym, nodes, rc, rgf, sampling_hops=2, num_samples=32, full_batch=True)
    assert pred.dtype == torch.bool and pred.shape == opred.shape and acc == f1 and 0.0 < of1 < 1.0
    flips = int((pred.cpu() != opred).sum())
    assert flips <= 3, flips                                  # logits agree to 1e-5: only entries at |logit| < 1e-5 may differ
    if flips == 0:
        assert f1 == of1
    tp_fp_fn = float((opred | (ym[torch.from_numpy(nodes)] > 0.5)).sum())
    assert abs(f1 - of1) <= 4.0 * (flips + 1e-9) / tp_fp_fn + 1e-12
    with pytest.raises(ValueError, match="training"):                          # autograd on the forced path: not built
        c(X.cuda(), g, large_graph=True)


def test_forced_large_path_refuses_an_over_budget_plan(monkeypatch):
    _cuda()
    from grapes_amd import full_graph
    from grapes_amd.eval import evaluate
    n = 6000
    indptr, indices, X, y, rc, rgf, c, gf, g, rng = _small(False, 100, 7, 64, 2)
    g.full_graph_plan()
    data = types.SimpleNamespace(x=X.cuda(), y=y.cuda())
    args = types.SimpleNamespace(sampling_hops=2, num_samples=64, use_indicators=True)
    monkeypatch.setattr(full_graph, "free_bytes", lambda device: 1 << 20)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match="GiB"):
        evaluate(c, gf, data, args, g, full_batch=True, large_graph=True)
    assert torch.cuda.memory_allocated() - before < 1 << 20                       # (nothing but the row list)


def test_row_list_with_repeated_hub_rows_past_the_item_cap():
    """grapes_gcn_large_aggregate over a row list that repeats a hub row until its items no longer fit below the plan's item cap
    (a distinct row list never needs more): the reservation stops at the cap, the rows that did not fit are walked by their own
    wavefront, GRAPES_STATUS_NODE_OVERFLOW is raised, and every output row equals that row's output over the distinct rows (bit for
    bit where it went through items, to fp32 rounding where the summation order changed)."""
    _cuda()
    from grapes_amd import ops
    indptr, indices, X, y, rc, rgf, c, gf, g, rng = _small(False, 100, 7, 64, 2)
    plan = g.full_graph_plan(hub_chunk=64)
    deg = np.diff(indptr)
    hub = int(deg.argmax())
    nc = -(-int(deg[hub]) // 64)
    assert nc >= 2 and plan.item_cap >= nc
    reps = plan.item_cap // nc + 3                                       # more copies of the hub than the cap holds items for
    others = rng.permutation(6000)[:300]
    rows_np = np.concatenate([np.full(reps, hub), others, np.full(3, hub)]).astype(np.int32)
    distinct = np.unique(rows_np)
    h = torch.randn(6000, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    b = torch.randn(16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.gcn_large_aggregate(h, plan, False, rows=torch.from_numpy(rows_np).cuda(), bias=b, relu=False, status=status)
    ref_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = ops.gcn_large_aggregate(h, plan, False, rows=torch.from_numpy(distinct.astype(np.int32)).cuda(), bias=b, status=ref_status)
    torch.cuda.synchronize()
    assert int(status) & 2 and int(ref_status) == 0
    expect = ref[torch.from_numpy(np.searchsorted(distinct, rows_np)).cuda()]
    scale = float(expect.abs().max())
    assert float((out - expect).abs().max()) <= 1e-6 * scale
    short = torch.from_numpy(deg[rows_np] <= 64).cuda()                 # rows without items: one wavefront either way
    assert torch.equal(out[short], expect[short])
    assert int((out == expect).all(dim=1).sum()) > int(short.sum())        # and the hub rows that did get items: bit-identical


# ---------------------------------------------------------------------------------------------- past the 2^31st entry
def _circulant(N, offsets, chunk=1 << 16):
    """CSR of row i -> (i + d) mod N for d in `offsets`, columns ascending, built on the device in row chunks."""
    k = len(offsets)
    d = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    rowptr = torch.arange(N + 1, dtype=torch.int64, device="cuda") * k
    col = torch.empty(N * k, dtype=torch.int32, device="cuda")
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        v = (torch.arange(lo, hi, device="cuda", dtype=torch.int64)[:, None] + d[None, :]) % N
        col[lo * k:hi * k] = torch.sort(v, dim=1).values.reshape(-1).to(torch.int32)
    return rowptr, col


def _window_sum(T, lo, hi):
    """S[i] = sum_{d=lo..hi} T[(i + d) mod N] in fp64 by prefix sums (T fp64 [N, f])."""
    N = T.shape[0]
    ext = torch.cat([T[N + lo:] if lo < 0 else T[:0], T, T[:hi] if hi > 0 else T[:0]])
    P = torch.zeros((ext.shape[0] + 1, T.shape[1]), dtype=torch.float64, device=T.device)
    torch.cumsum(ext, 0, out=P[1:])
    w = hi - lo + 1
    return P[w:w + N] - P[:N]


@pytest.mark.parametrize("directed,hub_chunk", [(False, None), (True, None), (False, 256)])
def test_circulant_beyond_2_31_entries_exact_reference(directed, hub_chunk):
    """hub_chunk=256: every 512-entry row is two work items, so the item path (lg_chunks_k, partials in chunk order) runs past
    the 2^31st entry too; the default chunk (1024) walks each row with its own wavefront."""
    _cuda()
    from grapes_amd.eval import evaluate
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    N, F, H, C = 4_400_000, 32, 64, 10
    offs = list(range(1, 513)) if directed else list(range(-256, 0)) + list(range(1, 257))
    rowptr, col = _circulant(N, offs)
    g = DeviceGraph(rowptr, col, N)
    assert g.nnz >= 2 ** 31 and int(rowptr[N - 1]) > 2 ** 31
    if hub_chunk is not None:                                   # (the first call fixes the plan's chunk)
        assert g.full_graph_plan(hub_chunk=hub_chunk).item_cap == 2 * N
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    X = torch.randn(N, F, device="cuda", generator=gen).mul_(16.0)          # (window means of O(1): logits of O(1))
    y = torch.randint(0, C, (N,), device="cuda", generator=gen)
    torch.manual_seed(12)
    c = GCN(F, [H, C]).cuda()
    with torch.no_grad():
        for p in c.parameters():
            if p.dim() == 1:
                p.uniform_(-0.05, 0.05)                                         # non-zero biases
    # fp64 reference: dinv = 513^-1/2 everywhere, Â = window sum / 513 (the window is i-256..i+256, or i-512..i for the transpose)
    lo, hi = (-512, 0) if directed else (-256, 256)
    W1, b1 = c.gcn_layers[0].lin.weight.double(), c.gcn_layers[0].bias.double()
    W2, b2 = c.gcn_layers[1].lin.weight.double(), c.gcn_layers[1].bias.double()
    with torch.no_grad():
        h1 = torch.relu(_window_sum(X.double(), lo, hi) / 513.0 @ W1.T + b1)
        ref = _window_sum(h1 @ W2.T, lo, hi) / 513.0 + b2
        del h1
    scale = max(1.0, float(ref.abs().max()))
    with torch.inference_mode():
        logits, _ = c(X, g)                                                     # automatic: nnz >= 2^31 - 1
    assert g.full_graph_plan().symmetric == (not directed)
    assert float((logits.double() - ref).abs().max()) <= 1e-5 * scale
    del logits
    data = types.SimpleNamespace(x=X, y=y)
    args = types.SimpleNamespace(sampling_hops=2, num_samples=16, use_indicators=True)
    acc, f1, pred = evaluate(c, None, data, args, g, full_batch=True, return_predictions=True)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 1e-5 * scale
    assert bool(clear.float().mean() > 0.99)
    assert torch.equal(pred[clear], ref.argmax(1)[clear])
    _, _, pred2 = evaluate(c, None, data, args, g, full_batch=True, return_predictions=True)
    assert torch.equal(pred, pred2)
    del g, rowptr, col, X, ref
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- papers100M at its real shape
def _two_hop_logits(rowptr, col, dinv, X, W1, b1, W2, b2, rows):
    """fp64 logits of `rows` from their two-hop neighbourhoods (symmetric graph without stored self-loops)."""
    dev = X.device

    def nbrs(r):
        beg, end = rowptr[r], rowptr[r + 1]
        cnt = end - beg
        seg = torch.repeat_interleave(torch.arange(r.numel(), device=dev), cnt)
        pos = torch.arange(int(cnt.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        return seg, col[beg[seg] + pos].long()

    seg, nb = nbrs(rows)
    u, inv = torch.unique(torch.cat([rows, nb]), return_inverse=True)
    s2, n2 = nbrs(u)
    dv = dinv.double()
    ax = torch.zeros((u.numel(), X.shape[1]), dtype=torch.float64, device=dev)
    for lo in range(0, n2.numel(), 1 << 22):
        sl = slice(lo, lo + (1 << 22))
        ax.index_add_(0, s2[sl], X[n2[sl]].double() * dv[n2[sl]][:, None])
    ax = dv[u][:, None] * (ax + dv[u][:, None] * X[u].double())
    t = torch.relu(ax @ W1.T + b1) @ W2.T
    r_idx, nb_idx = inv[:rows.numel()], inv[rows.numel():]
    out = torch.zeros((rows.numel(), t.shape[1]), dtype=torch.float64, device=dev)
    out.index_add_(0, seg, t[nb_idx] * dv[nb][:, None])
    return dv[rows][:, None] * (out + dv[rows][:, None] * t[r_idx]) + b2


def test_papers100m_full_batch_eval_real_shape(monkeypatch):
    _cuda()
    from grapes_amd import full_graph, synth
    from grapes_amd.eval import evaluate
    from grapes_amd.graph import DeviceGraph
    from grapes_amd.modules.gcn import GCN
    N, deg, maxdeg, F, C, *_ = synth.CONFIGS["papers100m"]
    rowptr, col = synth.synth_graph_device_chunked(N, deg, maxdeg, seed=0, device="cuda")
    g = DeviceGraph(rowptr, col, N)
    assert g.nnz > 3_000_000_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    X = synth.randn_rows_(torch.empty(N, F, device="cuda"), generator=gen)
    y = torch.randint(0, C, (N,), device="cuda", generator=gen)
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[torch.randperm(N, device="cuda", generator=gen)[:10_000_000]] = True
    torch.manual_seed(0)
    c = GCN(F, [256, C]).cuda()                                                 # main.py:162
    data = types.SimpleNamespace(x=X, y=y)
    args = types.SimpleNamespace(sampling_hops=3, num_samples=256, use_indicators=True)
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    acc, f1, pred = evaluate(c, None, data, args, g, mask=mask, full_batch=True, return_predictions=True)
    peak_extra = torch.cuda.max_memory_allocated() - base
    assert peak_extra <= N * 176 * 4 + 8 * 2 ** 30, peak_extra
    assert pred.numel() == 10_000_000 and 0.0 <= acc <= 1.0 and acc == f1
    # >= 256 sampled mask rows, half of them with CSR entries beyond the 2^31st, against fp64 two-hop logits
    rows = torch.nonzero(mask).reshape(-1)
    late = rows[rowptr[rows + 1] > 2 ** 31]
    early = rows[rowptr[rows + 1] <= 2 ** 31]
    pick_l = late[torch.randperm(late.numel(), device="cuda", generator=gen)[:128]]
    pick_e = early[torch.randperm(early.numel(), device="cuda", generator=gen)[:128]]
    pick = torch.cat([pick_e, pick_l])
    plan = g.full_graph_plan()
    assert plan.symmetric
    W1, b1 = c.gcn_layers[0].lin.weight.detach().double(), c.gcn_layers[0].bias.detach().double()
    W2, b2 = c.gcn_layers[1].lin.weight.detach().double(), c.gcn_layers[1].bias.detach().double()
    with torch.no_grad():
        # dinv from the row lengths, independent of the code under test (the synthetic CSR stores no self-loops)
        dinv_ref = (rowptr[1:] - rowptr[:-1] + 1).double().rsqrt()
        ref = _two_hop_logits(rowptr, col, dinv_ref, X, W1, b1, W2, b2, pick)
    scale = max(1.0, float(ref.abs().max()))
    pos = torch.searchsorted(rows, pick)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 1e-5 * scale
    assert int(clear[128:].sum()) >= 100 and int(clear[:128].sum()) >= 100
    assert torch.equal(pred[pos][clear], ref.argmax(1)[clear])
    # an over-budget plan (the bench's 3-layer classifier, N x 256 + N x 172 next to X, against a 1 GiB budget) is refused up front
    c3 = GCN(F, [256, 256, C]).cuda()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 30, 288 << 30))
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with pytest.raises(MemoryError, match="GiB"):
        evaluate(c3, None, data, args, g, mask=mask, full_batch=True)
    assert torch.cuda.max_memory_allocated() - before < 2 ** 30                 # (the mask's row list at most: nothing launched)
    del g, rowptr, col, X, plan
    torch.cuda.empty_cache()


def test_cli_papers100m_reaches_its_evaluations():
    _cuda()
    cmd = [sys.executable, "-m", "grapes_amd.main", "--dataset", "papers100m", "--max_epochs", "1", "--max_steps", "4",
           "--runs", "1", "--eval_frequency", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "valid_f1=" in r.stdout and "test_f1=" in r.stdout, r.stdout[-3000:]
