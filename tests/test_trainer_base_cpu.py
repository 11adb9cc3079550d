"""The trainers' shared base without a GPU: ``trainer.Trainer`` holds the plumbing both trainers used to repeat, once;
``rollouts.RolloutRunner`` is the rollout without a loss that ``ReinforceTrainer`` is and ``SupervisedTrainer`` keeps for
its evaluations; the loop of ``run`` re-iterates its batches and leaves process groups it did not create alone."""
from types import SimpleNamespace

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd.rollouts import RolloutRunner
from jolineedle_amd.trainer import Trainer
from tests.test_class_rollout_cpu import _NoEngine


def test_shared_plumbing_has_one_definition():
    assert issubclass(ja.ReinforceTrainer, Trainer) and issubclass(ja.SupervisedTrainer, Trainer)
    for cls in (ja.ReinforceTrainer, ja.SupervisedTrainer):
        for name in ("ddp_setup", "init_detection", "_grad_arena", "yolox_model"):
            assert name not in vars(cls), (cls.__name__, name)
            assert name in vars(Trainer)
    assert issubclass(ja.ReinforceTrainer, RolloutRunner)
    assert not issubclass(ja.SupervisedTrainer, RolloutRunner)


@pytest.mark.parametrize("test_len, want", [(9, 9), (None, 4), ("absent", 4)])
def test_supervised_eval_runner_is_a_rollout_runner_without_a_loss(test_len, want):
    kw = {} if test_len == "absent" else {"test_max_seq_len": test_len}
    sup = ja.SupervisedTrainer(ja.CfgNode(patch_size=64, max_seq_len=4, stop_enabled=True, seed=5, **kw), _NoEngine())
    runner = sup._eval_runner()
    assert isinstance(runner, RolloutRunner) and not isinstance(runner, ja.ReinforceTrainer)
    assert runner.max_ep_len == want and runner.stop_enabled is True and runner.seed == 5
    assert sup._eval_runner() is runner
    assert not hasattr(runner, "compute_metrics") and not hasattr(runner, "last_return_values")


class _Optimizer:
    sync_gradients = None


class _Model:
    device = torch.device("cpu")
    patch_size = 64

    def configure_optimizers(self, config):
        return _Optimizer(), _Optimizer()


class _Recording(Trainer):
    """``run`` as the trainers write it: what differs is handed to ``_run_loop``."""

    def run(self, rank, world_size, port, batches=None, max_iters=None, backend=None, flag="asked"):
        self.seen = []

        def step(i, batch, optim_gpt, optim_yolox):
            self.seen.append((i, batch, optim_gpt, optim_yolox))
            return len(self.seen)
        return self._run_loop(step, rank, world_size, port, backend, batches, max_iters, augment=False, sync_gradients=flag)


def test_run_loop_reiterates_batches_and_touches_no_process_group(monkeypatch):
    import torch.distributed as dist

    def boom(*a, **k):
        raise AssertionError("a process group was created or destroyed")
    monkeypatch.setattr(dist, "init_process_group", boom)
    monkeypatch.setattr(dist, "destroy_process_group", boom)
    a, b = {"image": "a"}, {"image": "b"}
    tr = _Recording(ja.CfgNode(max_iters=1), _Model())
    assert tr.run(3, 1, 29500, batches=[a, b], max_iters=5) == 5                 # the last step's value
    assert [s[1] for s in tr.seen] == [a, b, a, b, a] and [s[0] for s in tr.seen] == [0, 1, 2, 3, 4]
    assert tr.rank == 3 and tr.detection_augment is None and not dist.is_initialized()
    assert all(s[2] is tr.optim_gpt and s[3] is tr.optim_yolox for s in tr.seen)
    assert tr.optim_gpt.sync_gradients == "asked" and tr.optim_yolox.sync_gradients == "asked"
    tr.train_dataset = [b]
    assert tr.run(0, 1, 29500, flag=False) == 1 and [s[1] for s in tr.seen] == [b]      # config.max_iters, train_dataset
    assert tr.optim_gpt.sync_gradients is False
    with pytest.raises(AssertionError, match="needs an iterable of collated batches"):
        _Recording(ja.CfgNode(), _Model()).run(0, 1, 29500)


def test_the_trainers_ask_for_their_own_flag_values(monkeypatch):
    asked = {}

    def fake_loop(self, step, rank, world_size, port, backend, batches, max_iters, augment, sync_gradients):
        asked[type(self).__name__] = (port, augment, sync_gradients)
    monkeypatch.setattr(Trainer, "_run_loop", fake_loop)
    cfg = ja.CfgNode(patch_size=64, max_seq_len=4, entropy_weight=0.01, stop_enabled=True, reward_norm=False,
                     detection_enabled=False, augment_detection=True)
    for world in (1, 2):
        ja.ReinforceTrainer(cfg, _Model()).run(0, world, ddp_port=1234, batches=[])
        ja.SupervisedTrainer(cfg, _Model()).run(0, world, port=4321, batches=[], seed=1)
        # REINFORCE: augmentation only with detection; its step averages the gradients itself, so never the optimisers
        assert asked == {"ReinforceTrainer": (1234, False, False), "SupervisedTrainer": (4321, True, world > 1)}


def test_yolox_model_is_none_without_a_detector():
    model = SimpleNamespace(device=torch.device("cpu"), patch_size=64)
    cfg = ja.CfgNode(patch_size=64, max_seq_len=4, entropy_weight=0.01, stop_enabled=True, reward_norm=False)
    assert ja.ReinforceTrainer(cfg, model).yolox_model() is None
    assert ja.SupervisedTrainer(cfg, model).yolox_model() is None
    model._yolox_view = detector = object()
    assert ja.ReinforceTrainer(cfg, model).yolox_model() is detector
