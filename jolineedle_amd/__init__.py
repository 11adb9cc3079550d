"""jolineedle_amd — MI355X-native glimpse-rollout engine behind JoliNeedle's operator API.

Python mirror of the reference interface for the rollout hot path:
``GPT``, ``NeedleYOLOX``, ``NeedleGeneralEnv``, ``ReinforceTrainer.rollout`` with the
reference's names, argument meaning and error behaviour, over the C ABI of
``libjnroll.so`` (include/jnroll.h).  There is no CPU fallback: the HIP library must be
built (``python -c 'import __graft_entry__ as g; g.build()'``) and a GPU present.
"""
from .common import Action, ACTION_DELTAS, ActionInfo, get_actions_info  # noqa: F401
from .config import CfgNode, get_args, args_to_config  # noqa: F401
from ._lib import load_library, LibraryNotBuilt  # noqa: F401
from .gpt import GPT  # noqa: F401
from .env import NeedleGeneralEnv  # noqa: F401
from .yolox import NeedleYOLOX  # noqa: F401
from .reinforce import ReinforceTrainer  # noqa: F401
from .supervised import SupervisedTrainer  # noqa: F401
from .data import padded_collate, synthetic_batch  # noqa: F401
from .augment import DetectionAugment  # noqa: F401
from .checkpoint import (save_config, config_from_file, save_checkpoint, load_checkpoint,  # noqa: F401
                         load_detection_checkpoint)
from .infer import infer_images, plan_chunks, pad_to_patch_multiple, load_bboxes  # noqa: F401
from .trajectory import NeedleSimpleEnv, teacher_action_sets, teacher_action_sets_device  # noqa: F401
from .trajectory import PhiloxDraws, teacher_walks, teacher_walks_device  # noqa: F401
from .views import ImageViews  # noqa: F401
from .detection import (patch_bboxes2full_image, rollout_boxes_to_image, merge_boxes, merge_boxes_batched,  # noqa: F401
                        compute_detection_metrics, detection_targets, detection_cells, detection_cells_device,
                        rollout_boxes_packed, pack_boxes, unpack_boxes,
                        merge_boxes_device, merge_boxes_batched_device, match_detections_device, average_precision_device,
                        map_50_device, compute_detection_metrics_device, pool_walk_detections,
                        pool_walk_detections_device, cell_targets, average_precision_segments_device, map_50_segments,
                        map_50_segments_device)

__all__ = ["GPT", "NeedleYOLOX", "NeedleGeneralEnv", "ReinforceTrainer", "SupervisedTrainer", "Action", "ACTION_DELTAS",
           "ActionInfo", "get_actions_info", "CfgNode", "get_args", "args_to_config", "load_library"]
