"""grapes_amd.full_batch's flags: the reference full-batch.py's defaults (:26-50), config-file precedence (:146-150) and the
model-type refusal.  Parsing only: no GPU."""
import pytest

REFERENCE_DEFAULTS = {                                       # full-batch.py:26-50
    "dataset": "cora", "sampling_hops": 2, "num_samples": 16, "lr_gc": 1e-3, "use_indicators": True, "lr_gf": 1e-4,
    "loss_coef": 1e4, "log_z_init": 0.0, "reg_param": 0.0, "dropout": 0.0, "model_type": "gcn", "hidden_dim": 256,
    "max_epochs": 30, "batch_size": 512, "eval_frequency": 5, "eval_on_cpu": False, "eval_full_batch": False, "runs": 10,
    "notes": None, "log_wandb": True, "config_file": None,
}


def test_defaults_equal_full_batch_py():
    from grapes_amd import full_batch
    args = vars(full_batch.parse_args([]))
    for k, v in REFERENCE_DEFAULTS.items():
        assert args[k] == v, (k, args[k], v)
    assert set(args) == set(REFERENCE_DEFAULTS) | {"seed", "large_graph"}
    assert args["seed"] is None and args["large_graph"] == "auto"


def test_config_file_is_read_first_and_the_command_line_wins(tmp_path):
    from grapes_amd import full_batch
    cfg = tmp_path / "fb.txt"
    cfg.write_text('--dataset "ogbn-arxiv"\n--hidden_dim 128\n--dropout 0.5\n--log_wandb false  # comment\n--lr_gc 0.01\n')
    args = full_batch.parse_args(["--config_file", str(cfg), "--hidden_dim", "64", "--eval_full_batch", "true"])
    assert args.dataset == "ogbn-arxiv" and args.dropout == 0.5 and args.log_wandb is False and args.lr_gc == 0.01
    assert args.hidden_dim == 64 and args.eval_full_batch is True            # the command line wins
    assert args.max_epochs == 30                                             # untouched: full-batch.py's default


def test_large_graph_flag_and_explicit_booleans():
    from grapes_amd import full_batch
    assert full_batch.parse_args(["--large_graph", "true"]).large_graph == "true"
    with pytest.raises(SystemExit):
        full_batch.parse_args(["--large_graph", "maybe"])
    assert full_batch.parse_args(["--use_indicators", "false"]).use_indicators is False


@pytest.mark.parametrize("model", ["gat", "sage"])
def test_other_model_types_are_refused(model):
    from grapes_amd import full_batch
    with pytest.raises(NotImplementedError, match="gcn"):
        full_batch.parse_args(["--model_type", model])
