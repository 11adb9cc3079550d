"""``RolloutRunner``: the rollout of the reference's trainer (src/reinforce.py:108-215) over ``jn_rollout``, without a
loss: the whole trajectory of the whole batch is enqueued on the current stream, with no host synchronisation until the
step count is read.  ``ReinforceTrainer`` is a runner with a loss on top; ``SupervisedTrainer`` keeps one to evaluate."""
import contextlib
import ctypes as C
from typing import Dict

import torch

from . import _lib
from ._lib import JnRolloutOut, check, ptr
from .env import NeedleGeneralEnv


def _keys_table(agent_keys, B: int):
    """The host table of ``jn_set_rollout_keys``: uint64 [B, 2] = (stream seed, stream index) from any [B, 2] integers
    (a seed is taken modulo 2**64, as the rollout seeds are)."""
    import numpy as np
    rows = agent_keys.tolist() if hasattr(agent_keys, "tolist") else list(agent_keys)
    tab = np.array([[int(s) & 0xFFFFFFFFFFFFFFFF, int(i)] for s, i in rows], dtype=np.uint64).reshape(-1, 2)
    assert tab.shape[0] == B, f"agent_keys must be [{B}, 2], got {list(tab.shape)}"
    return np.ascontiguousarray(tab)


def _classes_table(classes, B: int):
    """The host table of ``jn_set_rollout_classes``: int64 [B] class ids from a [B] integer tensor (any device: one
    readback) or sequence.  An id outside ``embed_class`` raises what ``GPT.forward`` raises."""
    import numpy as np
    rows = classes.detach().reshape(-1).tolist() if torch.is_tensor(classes) else list(classes)
    tab = np.ascontiguousarray(np.array([int(c) for c in rows], dtype=np.int64).reshape(-1))
    assert tab.shape[0] == B, f"classes must be [{B}], got {list(tab.shape)}"
    assert int(tab.min()) >= 0 and int(tab.max()) < 100, "class id outside embed_class (100 rows)"
    return tab


ACTION_MASKS = {None: 0, "grid": 1, "unvisited": 2}      # the policies of ``jn_set_rollout_action_mask``


def _mask_policy(action_mask) -> int:
    if action_mask not in ACTION_MASKS:
        raise ValueError(f"action_mask must be None, 'grid' or 'unvisited', got {action_mask!r}")
    return ACTION_MASKS[action_mask]


class _RolloutGraph(torch.autograd.Function):
    """Graph node behind ``rollout()["logprobs"]`` / ``["entropies"]`` of a train-mode rollout ("carry
    autograd graph in training").  backward = ``jn_reinforce_backward`` with the upstream gradients torch hands over, then
    the engine's packed gradients are added to ``param.grad`` (reference layout)."""

    @staticmethod
    def forward(ctx, anchor, model, gen, logprobs, entropies, keep):
        # `keep`: every buffer the engine's backward reads through raw pointers (logits, actions, positions, final_emb,
        # masks, ..., forced actions) — held here so that the caching allocator cannot hand them out again when the
        # caller drops the rollout dict before loss.backward()
        ctx.model, ctx.gen, ctx.keep = model, gen, keep
        return logprobs.view_as(logprobs), entropies.view_as(entropies)

    @staticmethod
    def backward(ctx, dlp, dent):
        model = ctx.model
        if ctx.gen != model._rollout_gen:
            raise RuntimeError("backward through a rollout whose activations were overwritten by a later train-mode rollout")
        eng, dev = model.engine(), model.device
        dlp = None if dlp is None else dlp.to(dev, torch.float32).contiguous()
        dent = None if dent is None else dent.to(dev, torch.float32).contiguous()
        check(eng.lib.jn_reinforce_backward(eng.handle, ptr(dlp), ptr(dent), _lib.current_stream(dev)), "jn_reinforce_backward")
        model.publish_engine_grads()
        return None, None, None, None, None, None


class _RolloutCall:
    """What one engine rollout needs, prepared the same way for ``RolloutRunner.rollout`` and
    ``ReinforceTrainer.train_iteration``: the checked per-agent tables, the bound engine, the output buffers behind a
    ``JnRolloutOut``, the mode with its device inputs, and — the runner's rollout counter moved on — the seed and the
    agent keys of that rollout number."""

    def __init__(self, runner, env, sample_actions, forced_actions, start_positions, agent_keys, classes, token_positions,
                 action_mask=None):
        model, dev = runner.model, runner.device
        B = env.batch_size
        self.classes = None if classes is None else _classes_table(classes, B)       # checked before any engine call
        self.mask_policy = _mask_policy(action_mask if action_mask is not None else getattr(runner, "action_mask", None))
        if token_positions is None:
            token_positions = "sequence" if getattr(model.config, "no_recurrent_embedding", False) else "recurrent"
        if token_positions not in ("sequence", "recurrent"):
            raise ValueError(f"token_positions must be 'sequence', 'recurrent' or None, got {token_positions!r}")
        self.by_token = token_positions == "sequence"
        if self.by_token and model.training and torch.is_grad_enabled():
            raise NotImplementedError(
                "token_positions='sequence' is for eval-mode rollouts: in train mode the reference re-encodes the whole "
                "prefix at every step with BatchNorm statistics over B*(t+1) patches, which the per-step rollout cannot "
                "reproduce (call model.eval() or torch.no_grad())")
        model.sync_weights()
        self.eng = eng = model.engine()
        env.bind(eng)
        T, C_, nA = env.max_ep_len, model.n_embd, eng.cfg.n_actions
        f32 = dict(device=dev, dtype=torch.float32)
        self.buf = {
            "rewards": torch.empty((B, T), **f32), "returns": torch.empty((B, T), **f32),
            "logprobs": torch.empty((B, T), **f32), "entropies": torch.empty((B, T), **f32),
            "masks": torch.empty((B, T + 1), device=dev, dtype=torch.uint8),
            "logit_masks": torch.empty((B, T), device=dev, dtype=torch.uint8),
            "positions": torch.empty((B, T + 1, 2), device=dev, dtype=torch.int64),
            "actions": torch.empty((B, T), device=dev, dtype=torch.int64),
            "logits": torch.empty((B, T, nA), **f32),
            "final_emb": torch.empty((B, T + 1, C_), **f32),
        }
        self.out = JnRolloutOut()
        for k, t in self.buf.items():
            setattr(self.out, k + "_dev", t.data_ptr())
        if forced_actions is not None:
            self.mode = _lib.JN_MODE_FORCED
            forced_actions = forced_actions.to(dev, torch.int64).contiguous()
        else:
            self.mode = _lib.JN_MODE_SAMPLE if sample_actions else _lib.JN_MODE_GREEDY
        if start_positions is not None:
            start_positions = start_positions.to(dev, torch.int64).contiguous()
        self.forced_actions, self.start_positions = forced_actions, start_positions
        runner._rollouts += 1
        self.seed = (runner.seed * 1000003 + runner._rollouts) & 0xFFFFFFFFFFFFFFFF
        self.keys = runner._agent_keys_table(agent_keys, B)
        self.stream = _lib.current_stream(dev)
        self.teacher = None       # (targets [B,Gh,Gw] or None, sets [B,T]) on the device once the caller wants the teacher
        # the action sets the decisions were made under, [B,T] uint16 bit patterns (torch has no dependable uint16)
        self.action_sets = torch.empty((B, T), device=dev, dtype=torch.int16) if self.mask_policy else None

    @contextlib.contextmanager
    def armed(self):
        """The engine's switches around the one engine call.  They are sticky in the engine: set for this rollout only,
        so that every other caller of the engine (and the default path, which makes none of these calls) finds it as it
        always was — armed with ``check``, disarmed unchecked on the way out, also when the engine call raised."""
        lib, h, B = self.eng.lib, self.eng.handle, len(self.buf["rewards"])
        switches = []             # (export, arming arguments, disarming arguments)
        if self.keys is not None:
            switches.append(("jn_set_rollout_keys", (self.keys.ctypes.data_as(C.c_void_p), B), (None, 0)))
        if self.classes is not None:
            switches.append(("jn_set_rollout_classes", (self.classes.ctypes.data_as(C.c_void_p), B), (None, 0)))
        if self.by_token:
            switches.append(("jn_set_rollout_positions", (1,), (0,)))
        if self.teacher is not None:
            switches.append(("jn_set_rollout_teacher", tuple(ptr(t) for t in self.teacher), (None, None)))
        if self.mask_policy:
            switches.append(("jn_set_rollout_action_mask", (self.mask_policy, ptr(self.action_sets)), (0, None)))
        try:
            for name, on, _ in switches:
                check(getattr(lib, name)(h, *on), name)
            yield
        finally:
            for name, _, off in switches:
                getattr(lib, name)(h, *off)


class RolloutRunner:
    """A model, the walk's length and STOP rule, and the numbered random streams of its rollouts: all ``rollout`` needs
    and all ``ragged`` / ``infer`` read of a trainer.  `agent_streams`: "batch", or "global" for
    ``dist.shard_agent_keys`` of this rank (checked at the rollout)."""

    def __init__(self, model, max_ep_len: int, stop_enabled: bool, seed: int = 0, rank: int = 0, agent_streams: str = "batch",
                 action_mask: str = None):
        self.model, self.device, self.patch_size = model, model.device, model.patch_size
        self.action_mask = action_mask      # what a rollout without an `action_mask` of its own runs under (config.action_mask)
        self.max_ep_len, self.stop_enabled, self.n_glimps_levels = max_ep_len, stop_enabled, 1
        self.seed, self.rank, self.agent_streams = int(seed), rank, agent_streams
        self._rollouts = 0

    def rollout(self, env: NeedleGeneralEnv, do_detection: bool = False, sample_actions: bool = True,
                forced_actions: torch.Tensor = None, start_positions: torch.Tensor = None,
                keep_patches: bool = True, stop_early: bool = True, bbox_lists: bool = True,
                token_positions: str = None, teacher: bool = False,
                teacher_targets: torch.Tensor = None, agent_keys=None, classes=None,
                action_mask: str = None) -> Dict[str, torch.Tensor]:
        """src/reinforce.py:108-215.  Extra keyword arguments (not in the reference):
        `forced_actions` [B,T] replays a trajectory, `start_positions` [B,2] injects reset
        positions (reference: env.reset(positions)), `keep_patches=False` skips the
        [B,S+1,3,P,P] patch stack, `stop_early=False` always runs max_ep_len steps, `bbox_lists=False` leaves
        "bboxes" empty (no B x (S+1) clones): the detections are then only "det_boxes" [B,S+1,K,7] / "det_counts"
        [B,S+1] on the device, which ``detection.rollout_boxes_to_image`` assembles per image.

        `token_positions`: "recurrent" gives every new token the 1-D position 0 (gpt.py:431-449, what a REINFORCE-trained
        policy saw), "sequence" gives the token of step t position t — the last row of the full-prefix forward
        (gpt.py:331-354) that a supervised policy was trained on and that ``--no-recurrent-embedding`` selects
        (gpt.py:427-428); None = "sequence" when ``model.config.no_recurrent_embedding``, else "recurrent".  "sequence"
        is an eval-mode feature (see the NotImplementedError below).
        `teacher=True` adds "teacher_sets" [B,S] uint8: per step the teacher's action set
        (``trajectory.teacher_action_sets``) of the state the decision saw, computed inside the rollout;
        `teacher_targets` [B,Gh,Gw] replaces the env's bbox masks as the cells the teacher walks to.
        `agent_keys` [B,2] integers (stream seed, stream index): agent b draws its sampled actions, and its random start
        when `start_positions` is None, from that Philox stream instead of (this rollout's seed, b)
        (``jn_set_rollout_keys``) — an agent then walks the same way wherever it sits in whichever batch; None = the
        default streams, or ``dist.shard_agent_keys`` of this rank when ``config.agent_streams == "global"``.
        `classes` [B] integers (a tensor on any device or a sequence): agent b's class token is row classes[b] of
        ``embed_class`` (``jn_set_rollout_classes``), what ``test_model_on_env`` feeds a class-conditioned policy
        (src/supervised.py:317-331); in train mode the class token's gradient goes to those rows, whenever the backward
        runs.  None = row 0 for every agent, the reference's REINFORCE loop (src/reinforce.py:128-129).
        `action_mask`: "grid" lets no decision pick a move that leaves the agent's grid, "unvisited" none that re-enters a
        visited cell while a fresh neighbour exists (``jn_set_rollout_action_mask``; not in the reference, whose env clamps):
        log-probs, entropies, the greedy choice and the samples are those of the softmax over the allowed actions, and
        "action_sets" [B,S] (int64, bit a = action a allowed) holds the sets.  In train mode the backward differentiates
        under the same sets.  None = ``config.action_mask`` (default None: no masking, no "action_sets")."""
        model, dev = self.model, self.device
        call = _RolloutCall(self, env, sample_actions, forced_actions, start_positions, agent_keys, classes, token_positions,
                            action_mask)
        eng, buf, out, stream = call.eng, call.buf, call.out, call.stream
        B, T, P = env.batch_size, env.max_ep_len, env.patch_size
        f32 = dict(device=dev, dtype=torch.float32)
        patches = torch.empty((B, T + 1, 3, P, P), **f32) if keep_patches else None
        out.patches_dev = patches.data_ptr() if patches is not None else None
        Kd = eng.cfg.max_det_per_patch
        if do_detection:
            det_boxes = torch.zeros((B, T + 1, Kd, 7), **f32)
            det_counts = torch.zeros((B, T + 1), device=dev, dtype=torch.int32)
            out.det_boxes_dev, out.det_counts_dev = det_boxes.data_ptr(), det_counts.data_ptr()
        # model.train() + grad mode (the reference's training loop, src/reinforce.py:304, 326): batch-statistics BatchNorm,
        # activations of every step kept resident, logprobs / entropies leave with a graph (autograd bridge)
        graph = bool(model.training) and torch.is_grad_enabled() and not do_detection
        sets = None
        if teacher:
            sets = torch.empty((B, T), device=dev, dtype=torch.uint8)
            if teacher_targets is not None:
                teacher_targets = teacher_targets.to(dev, torch.uint8).contiguous()
                grid = (B, env.n_vertical_patches, env.n_horizontal_patches)
                assert tuple(teacher_targets.shape) == grid, f"teacher_targets must be {grid}, got {tuple(teacher_targets.shape)}"
            call.teacher = (teacher_targets, sets)
        with call.armed():
            if graph:
                model.bind_flat()
                model._rollout_gen += 1
                check(eng.lib.jn_reinforce_forward(eng.handle, call.mode, ptr(call.forced_actions), ptr(call.start_positions),
                                                   call.seed, int(stop_early), C.byref(out), stream), "jn_reinforce_forward")
                anchor = next(p for p in model.parameters() if p.requires_grad)
                keep = dict(buf, forced_actions=call.forced_actions, start_positions=call.start_positions)
                buf["logprobs"], buf["entropies"] = _RolloutGraph.apply(anchor, model, model._rollout_gen, buf["logprobs"],
                                                                        buf["entropies"], keep)
            else:
                check(eng.lib.jn_rollout(eng.handle, call.mode, ptr(call.forced_actions), ptr(call.start_positions), call.seed,
                                         int(do_detection), int(stop_early), C.byref(out), stream), "jn_rollout")
        S = C.c_int()
        check(eng.lib.jn_rollout_steps(eng.handle, C.byref(S), stream), "jn_rollout_steps")
        S = S.value
        res = {
            "rewards": buf["rewards"][:, :S], "returns": buf["returns"][:, :S],
            "logprobs": buf["logprobs"][:, :S], "entropies": buf["entropies"][:, :S],
            "masks": buf["masks"][:, :S + 1].bool(), "logit_masks": buf["logit_masks"][:, :S].bool(),
            "positions": buf["positions"][:, :S + 1], "bboxes": [[] for _ in range(B)],
            "det_counts": det_counts[:, :S + 1] if do_detection else None,
            "det_boxes": det_boxes[:, :S + 1] if do_detection else None,
            "patches": patches[:, :S + 1] if patches is not None else None,
            "actions": buf["actions"][:, :S], "logits": buf["logits"][:, :S],
            "final_emb": buf["final_emb"][:, :S + 1],
        }
        if teacher:
            res["teacher_sets"] = sets[:, :S]
        if call.action_sets is not None:
            res["action_sets"] = call.action_sets[:, :S].to(torch.int64) & 0xFFFF
        if do_detection and bbox_lists:       # ragged list-of-lists of [n,7] | None (src/reinforce.py:145-146, 166-167)
            cnt = det_counts[:, :S + 1].tolist()
            res["bboxes"] = [[det_boxes[b, t, :cnt[b][t]].clone() if cnt[b][t] > 0 else None for t in range(S + 1)]
                             for b in range(B)]
        return res

    def _agent_keys_table(self, agent_keys, B: int):
        """uint64 [B, 2] host table for the rollout numbered ``self._rollouts``, or None (no ``jn_set_rollout_keys`` call):
        the caller's `agent_keys`, else with ``agent_streams == "global"`` this rank's ``dist.shard_agent_keys``."""
        mode = self.agent_streams
        if mode not in ("batch", "global"):
            raise ValueError(f"config.agent_streams must be 'batch' or 'global', got {mode!r}")
        if agent_keys is None and mode == "global":
            import torch.distributed as dist
            from .dist import shard_agent_keys
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
            agent_keys = shard_agent_keys(self.seed, self._rollouts, int(self.rank), world, B)
        return None if agent_keys is None else _keys_table(agent_keys, B)
