"""CPU checks of what the six drivers share (grapes_amd/driver.py, target_batch.py, modules/sampling.py): every driver's parsed
namespace against literal dicts recorded from the drivers when each carried its own parser, their refusals with the messages of
that time, the samplers' status messages, and graphsaint._f1 against the function it was."""
import importlib
from types import SimpleNamespace

import pytest
import torch

_MAIN_DEFAULTS = {
    'dataset': 'cora', 'sampling_hops': 2, 'num_samples': 16, 'use_indicators': True, 'lr_gf': 0.0001, 'lr_gc': 0.001,
    'loss_coef': 10000.0, 'log_z_init': 0.0, 'reg_param': 0.0, 'dropout': 0.0, 'model_type': 'gcn', 'hidden_dim': 256,
    'embed_nodes': False, 'node_emb_dim': 64, 'max_epochs': 30, 'batch_size': 512, 'eval_frequency': 5, 'eval_on_cpu': True,
    'eval_full_batch': True, 'random_sampling': False, 'runs': 10, 'split_id': 0, 'seed': None, 'notes': None, 'log_wandb': False,
    'config_file': None, 'reinforce_baseline': False, 'e_cap': 131072, 'max_steps': None, 'engine': 'auto', 'pipeline': True,
    'classifier': 'gcn', 'gcn2_alpha': 0.1, 'gcn2_theta': 0.5, 'gcn2_shared_weights': True, 'pna_aggregators': 'mean,min,max,std',
    'pna_scalers': 'identity,amplification,attenuation', 'gat_heads': 1}
_FULL_BATCH_DEFAULTS = {
    'dataset': 'cora', 'sampling_hops': 2, 'num_samples': 16, 'lr_gc': 0.001, 'use_indicators': True, 'lr_gf': 0.0001,
    'loss_coef': 10000.0, 'log_z_init': 0.0, 'reg_param': 0.0, 'dropout': 0.0, 'model_type': 'gcn', 'hidden_dim': 256,
    'max_epochs': 30, 'batch_size': 512, 'eval_frequency': 5, 'eval_on_cpu': False, 'eval_full_batch': False, 'runs': 10,
    'notes': None, 'log_wandb': True, 'config_file': None, 'seed': None, 'large_graph': 'auto'}
_GRAPHSAINT_DEFAULTS = {
    'use_normalization': False, 'hidden_dim': 256, 'dataset': 'cora', 'runs': 1, 'lr': 0.01, 'max_epoch': 50, 'embed_nodes': False,
    'node_emb_dim': 64, 'batch_size': 256, 'walk_length': 2, 'num_steps': 1, 'seed': None, 'engine': 'graph', 'e_cap': None,
    'large_graph': 'auto', 'sampler': 'rw', 'sample_coverage': 0}
_TARGET_BATCH_DEFAULTS = {
    'dataset': 'cora', 'batch_size': 512, 'hidden_dim': 256, 'num_layers': 2, 'lr': 0.001, 'max_epoch': 100, 'eval_frequency': 1,
    'dropout': 0.0, 'runs': 1, 'seed': None}
_LADIES_DEFAULTS = dict(_TARGET_BATCH_DEFAULTS, sampler='ladies', samp_num=64, e_cap=None)
_ASGCN_DEFAULTS = dict(_TARGET_BATCH_DEFAULTS, samp_num=64, e_cap=None, var_coef=0.5)
_GRAPHSAGE_DEFAULTS = dict(_TARGET_BATCH_DEFAULTS, fanouts=[25, 10], aggr='mean')

# one non-default value per flag (--model_type and --config_file apart: the first takes gcn alone, the second names a file)
_CLASSIFIER_ARGV = ["--dataset", "arxiv", "--sampling_hops", "3", "--num_samples", "8", "--use_indicators", "false", "--lr_gf", "0.001",
                    "--lr_gc", "0.01", "--loss_coef", "10.0", "--log_z_init", "1.0", "--reg_param", "0.5", "--dropout", "0.1",
                    "--hidden_dim", "64", "--max_epochs", "3", "--batch_size", "128", "--eval_frequency", "2", "--runs", "2",
                    "--notes", "hi", "--seed", "7", "--classifier", "gcn2", "--gcn2_alpha", "0.2", "--gcn2_theta", "0.6",
                    "--gcn2_shared_weights", "false", "--pna_aggregators", "mean", "--pna_scalers", "identity", "--gat_heads", "2"]
_CLASSIFIER_SET = {
    'dataset': 'arxiv', 'sampling_hops': 3, 'num_samples': 8, 'use_indicators': False, 'lr_gf': 0.001, 'lr_gc': 0.01,
    'loss_coef': 10.0, 'log_z_init': 1.0, 'reg_param': 0.5, 'dropout': 0.1, 'model_type': 'gcn', 'hidden_dim': 64, 'max_epochs': 3,
    'batch_size': 128, 'eval_frequency': 2, 'runs': 2, 'notes': 'hi', 'seed': 7, 'config_file': None, 'classifier': 'gcn2',
    'gcn2_alpha': 0.2, 'gcn2_theta': 0.6, 'gcn2_shared_weights': False, 'pna_aggregators': 'mean', 'pna_scalers': 'identity',
    'gat_heads': 2}
_TARGET_BATCH_ARGV = ["--dataset", "arxiv", "--batch_size", "128", "--hidden_dim", "64", "--num_layers", "3", "--lr", "0.01",
                      "--max_epoch", "5", "--eval_frequency", "2", "--dropout", "0.1", "--runs", "2", "--seed", "7"]
_TARGET_BATCH_SET = {
    'dataset': 'arxiv', 'batch_size': 128, 'hidden_dim': 64, 'num_layers': 3, 'lr': 0.01, 'max_epoch': 5, 'eval_frequency': 2,
    'dropout': 0.1, 'runs': 2, 'seed': 7}

NAMESPACES = [
    ("main", ["--dataset", "cora"], _MAIN_DEFAULTS),
    ("main", _CLASSIFIER_ARGV + ["--embed_nodes", "true", "--node_emb_dim", "32", "--eval_on_cpu", "false", "--eval_full_batch", "false",
                                 "--random_sampling", "true", "--split_id", "1", "--log_wandb", "true", "--reinforce_baseline", "true",
                                 "--e_cap", "4096", "--max_steps", "4", "--engine", "eager", "--pipeline", "false"],
     dict(_CLASSIFIER_SET, embed_nodes=True, node_emb_dim=32, eval_on_cpu=False, eval_full_batch=False, random_sampling=True,
          split_id=1, log_wandb=True, reinforce_baseline=True, e_cap=4096, max_steps=4, engine='eager', pipeline=False)),
    ("full_batch", [], _FULL_BATCH_DEFAULTS),
    ("full_batch", _CLASSIFIER_ARGV + ["--eval_on_cpu", "true", "--eval_full_batch", "true", "--log_wandb", "false",
                                       "--large_graph", "false"],
     dict(_CLASSIFIER_SET, eval_on_cpu=True, eval_full_batch=True, log_wandb=False, large_graph='false')),
    ("graphsaint", ["--dataset", "cora"], _GRAPHSAINT_DEFAULTS),
    ("graphsaint", ["--dataset", "arxiv", "--use_normalization", "--hidden_dim", "64", "--runs", "2", "--lr", "0.1", "--max_epoch", "5",
                    "--embed_nodes", "true", "--node_emb_dim", "32", "--batch_size", "128", "--walk_length", "3", "--num_steps", "4",
                    "--seed", "7", "--engine", "eager", "--e_cap", "1000", "--large_graph", "true", "--sampler", "edge",
                    "--sample_coverage", "2"],
     {'use_normalization': True, 'hidden_dim': 64, 'dataset': 'arxiv', 'runs': 2, 'lr': 0.1, 'max_epoch': 5, 'embed_nodes': True,
      'node_emb_dim': 32, 'batch_size': 128, 'walk_length': 3, 'num_steps': 4, 'seed': 7, 'engine': 'eager', 'e_cap': 1000,
      'large_graph': 'true', 'sampler': 'edge', 'sample_coverage': 2}),
    ("ladies", ["--dataset", "cora"], _LADIES_DEFAULTS),
    ("ladies", _TARGET_BATCH_ARGV + ["--sampler", "fastgcn", "--samp_num", "32", "--e_cap", "1000"],
     dict(_TARGET_BATCH_SET, sampler='fastgcn', samp_num=32, e_cap=1000)),
    ("asgcn", ["--dataset", "cora"], _ASGCN_DEFAULTS),
    ("asgcn", _TARGET_BATCH_ARGV + ["--samp_num", "32", "--e_cap", "1000", "--var_coef", "0.25"],
     dict(_TARGET_BATCH_SET, samp_num=32, e_cap=1000, var_coef=0.25)),
    ("graphsage", ["--dataset", "cora"], _GRAPHSAGE_DEFAULTS),
    ("graphsage", _TARGET_BATCH_ARGV + ["--fanouts", "5,-1,3", "--aggr", "sum"], dict(_TARGET_BATCH_SET, fanouts=[5, -1, 3], aggr='sum')),
]


def _driver(name):
    return importlib.import_module("grapes_amd." + name)


@pytest.mark.parametrize("name,argv,want", NAMESPACES,
                         ids=[f"{n}-{'set' if len(a) > 2 else 'defaults'}" for n, a, _ in NAMESPACES])
def test_parsed_namespace_is_the_recorded_one(name, argv, want):
    got = vars(_driver(name).parse_args(argv))
    assert got == want
    assert all(type(got[k]) is type(want[k]) for k in want)               # (1 == 1.0 == True: the types are pinned too)


_BATCH_LADIES = "--num_layers, --samp_num and --eval_frequency are at least 1, --batch_size is 1 .. 4096"
_BATCH_SAGE = "--eval_frequency and --hidden_dim are at least 1, --batch_size is 1 .. 4096"
REFUSALS = [
    ("graphsaint", [], SystemExit, "--dataset is required"),
    ("ladies", [], SystemExit, "--dataset is required"),
    ("asgcn", [], SystemExit, "--dataset is required"),
    ("graphsage", [], SystemExit, "--dataset is required"),
    ("ladies", ["--dataset", "cora", "--batch_size", "5000"], ValueError, _BATCH_LADIES),
    ("ladies", ["--dataset", "cora", "--batch_size", "0"], ValueError, _BATCH_LADIES),
    ("ladies", ["--dataset", "cora", "--samp_num", "0"], ValueError, _BATCH_LADIES),
    ("ladies", ["--dataset", "cora", "--num_layers", "0"], ValueError, _BATCH_LADIES),
    ("asgcn", ["--dataset", "cora", "--batch_size", "5000"], ValueError, _BATCH_LADIES),
    ("asgcn", ["--dataset", "cora", "--eval_frequency", "0"], ValueError, _BATCH_LADIES),
    ("asgcn", ["--dataset", "cora", "--var_coef", "-1"], ValueError, "--var_coef is not negative"),
    ("graphsage", ["--dataset", "cora", "--batch_size", "5000"], ValueError, _BATCH_SAGE),
    ("graphsage", ["--dataset", "cora", "--hidden_dim", "0"], ValueError, _BATCH_SAGE),
    ("graphsage", ["--dataset", "cora", "--fanouts", "25,10", "--num_layers", "3"], ValueError,
     "--fanouts holds one entry per layer: 2 given for --num_layers 3"),
    # (the fanouts are judged before the ranges, as they were)
    ("graphsage", ["--dataset", "cora", "--fanouts", "25,10", "--num_layers", "3", "--batch_size", "5000"], ValueError,
     "--fanouts holds one entry per layer: 2 given for --num_layers 3"),
    ("graphsage", ["--dataset", "cora", "--fanouts", "65"], ValueError,
     "NeighborSampler: fanout 65 is not built (-1 for every neighbour, or 1 .. 64)"),
    ("graphsaint", ["--dataset", "cora", "--sample_coverage", "3"], ValueError,
     "--sample_coverage K (K > 0) goes with --use_normalization: the estimate is read by the normalised step alone"),
    ("main", ["--model_type", "gat"], NotImplementedError,
     "only model_type=gcn is built (the reference's other model classes are dead code)"),
    ("full_batch", ["--model_type", "gat"], NotImplementedError,
     "only model_type=gcn is built (full-batch.py:72-73 builds no other model)"),
]


@pytest.mark.parametrize("name,argv,exc,message", REFUSALS)
def test_refusals_keep_their_type_and_words(name, argv, exc, message):
    with pytest.raises(exc) as e:
        _driver(name).parse_args(argv)
    assert str(e.value) == message


def test_unknown_choices_leave_through_argparse():
    for name, argv in (("ladies", ["--sampler", "asgcn"]), ("asgcn", ["--sampler", "ladies"]), ("graphsage", ["--aggr", "max"]),
                       ("graphsage", ["--fanouts", "10,x"])):
        with pytest.raises(SystemExit):
            _driver(name).parse_args(["--dataset", "cora"] + argv)


# ------------------------------------------------------------------------------------------------ status words
def _with_status(cls, word, **fields):
    """An instance of a sampler class as check() reads it: the status word and the graph's two bitmaps, on the host."""
    s = cls.__new__(cls)
    s.status = torch.tensor([word], dtype=torch.int32)
    s.graph = SimpleNamespace(bits=torch.ones(3, dtype=torch.int64), prev_bits=torch.ones(3, dtype=torch.int64))
    for k, v in fields.items():
        setattr(s, k, v)
    return s


STATUS_MESSAGES = [
    ("ladies", 1, "ladies sampler: edge buffer overflow (raise e_cap)"),
    ("ladies", 2, "ladies sampler: node buffer overflow"),
    ("ladies", 4, "ladies sampler: index out of range"),
    ("ladies", 5, "ladies sampler: edge buffer overflow (raise e_cap), index out of range"),
    ("fastgcn", 5, "fastgcn sampler: edge buffer overflow (raise e_cap), index out of range"),
    ("asgcn", 1, "asgcn sampler: edge buffer overflow (raise e_cap)"),
    ("sage", 1, "neighbour sampler: edge buffer overflow"),
    ("sage", 2, "neighbour sampler: node buffer overflow"),
    ("sage", 4, "neighbour sampler: index out of range"),
    ("sage", 5, "neighbour sampler: edge buffer overflow, index out of range"),
    ("saint", 1, "GraphSAINT sampler: edge buffer overflow (raise e_cap)"),
    ("saint", 2, "GraphSAINT sampler: "),
    ("saint", 4, "GraphSAINT sampler: index out of range"),
    ("saint", 5, "GraphSAINT sampler: edge buffer overflow (raise e_cap), index out of range"),
]


@pytest.mark.parametrize("who,word,message", STATUS_MESSAGES)
def test_samplers_raise_their_status_messages(who, word, message):
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.ladies import LayerWiseSampler
    from grapes_amd.modules.sage import NeighborSampler
    from grapes_amd.modules.saint import GraphSAINTNodeSampler
    if who == "sage":
        s = _with_status(NeighborSampler, word)
    elif who == "saint":
        s = _with_status(GraphSAINTNodeSampler, word)
    elif who == "asgcn":                                                  # (AdaptiveSampler's check() is LayerWiseSampler's, named by _name)
        s = _with_status(LayerWiseSampler, word, kind="ladies", _name="asgcn")
    else:
        s = _with_status(LayerWiseSampler, word, kind=who)
    with pytest.raises(GrapesHipError) as e:
        s.check()
    assert str(e.value) == message
    assert int(s.status) == 0                                             # cleared: the next check() passes
    s.check()
    marked = who == "saint"                                               # GraphSAINT's batches leave the bitmaps alone
    assert bool(s.graph.bits.any()) == marked and bool(s.graph.prev_bits.any()) == marked


def test_raise_on_status_passes_a_clear_word_and_works_without_a_graph():
    from grapes_amd._lib import GrapesHipError
    from grapes_amd.modules.sampling import raise_on_status
    status = torch.zeros(1, dtype=torch.int32)
    raise_on_status(status, "anything")
    status[0] = 7
    with pytest.raises(GrapesHipError) as e:
        raise_on_status(status, "hop")
    assert str(e.value) == "hop: edge buffer overflow, node buffer overflow, index out of range" and int(status) == 0


def test_draw_seed_consumes_the_generator_only_for_none():
    from grapes_amd.modules.sampling import draw_seed
    torch.manual_seed(11)
    want = int(torch.randint(0, 2 ** 62, (1,)).item())
    after = torch.rand(1)
    torch.manual_seed(11)
    assert draw_seed(5) == 5 and draw_seed(None) == want and torch.equal(torch.rand(1), after)


# ------------------------------------------------------------------------------------------------ micro-F1
def _f1_as_it_was(y_pred, y_true) -> float:
    tp = int((y_true & y_pred).sum()); fp = int((~y_true & y_pred).sum()); fn = int((y_true & ~y_pred).sum())
    try:
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        return 2 * (precision * recall) / (precision + recall)
    except ZeroDivisionError:
        return 0.0


def test_f1_through_eval_metrics_is_the_function_it_was():
    from grapes_amd.graphsaint import _f1
    gen = torch.Generator().manual_seed(0)
    cases = []
    for n, c, p in ((1, 1, 0.5), (7, 3, 0.5), (64, 5, 0.1), (33, 12, 0.9), (200, 40, 0.3)):
        pred, true = torch.rand(n, c, generator=gen) < p, torch.rand(n, c, generator=gen) < 0.4
        cases += [(pred, true), (torch.zeros_like(pred), true), (pred, torch.zeros_like(true)),
                  (torch.zeros_like(pred), torch.zeros_like(true)), (true, true), (~true, true)]
    for pred, true in cases:
        assert _f1(pred, true) == _f1_as_it_was(pred, true)
    assert any(_f1_as_it_was(p, t) not in (0.0, 1.0) for p, t in cases)
