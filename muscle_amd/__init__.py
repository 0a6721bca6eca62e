"""muscle_amd — MI355X-native MCL / MuSCLe training hot path.

Public names mirror the reference's `src/__init__.py:1-6` for the path that is built: the MuSCLe model (CAM-encoder
and decoder modes), the MCL loss callables, `edge.FieldLoss`, the loop bodies (`mcl_step`, `muscle_step`) and the fused
optimiser; `muscle_amd.infer` (CAM generation), `muscle_amd.evaluation` (per-epoch mIoU sweep) and
`muscle_amd.indexing` (IRN random walk) and `muscle_amd.irn` (the IRN network, `EdgeDisplacement`, and `infer_irn`) cover the scripts around the training loop.  Importing the package never needs
a GPU; running anything does.
"""
from .MuSCLe import MuSCLe  # noqa: F401
from .loss_multilabel import (FocalLoss, Log_Sum_Exp_Pairwise_Loss, MultiLabelSoftMarginLoss,  # noqa: F401
                              image_level_contrast)
from .optim import FusedAdam  # noqa: F401
from .train_step import cam_softmaxnorm, er_loss, mcl_step, muscle_step  # noqa: F401
from . import edge  # noqa: F401
from .phase2 import EMD, PixPro, cam_maxnorm, get_dynamic_crops  # noqa: F401
from . import phase2 as torchutils  # noqa: F401  (reference name of the module holding get_dynamic_crops)

__all__ = ["MuSCLe", "FocalLoss", "Log_Sum_Exp_Pairwise_Loss", "MultiLabelSoftMarginLoss", "image_level_contrast",
           "FusedAdam", "cam_softmaxnorm", "er_loss", "mcl_step", "EMD", "PixPro", "cam_maxnorm", "get_dynamic_crops",
           "torchutils", "edge", "muscle_step"]
from .graph import GraphedMuscleStep, GraphedStep  # noqa: F401,E402
from .ops import get_gemm_mode, set_gemm_mode  # noqa: F401,E402
from . import data  # noqa: F401,E402  (input path: two-view sampler + device-side color_norm / crop stage)
from .irn import EdgeDisplacement  # noqa: F401,E402  (the IRN edge / displacement network of infer_irn.py)
from .irn import AffinityDisplacementLoss, irn_step  # noqa: F401,E402  (training the IRN heads; script: muscle_amd.train_irn)
from .optim import PolyOptimizer  # noqa: F401,E402
from .crf import crf_inference_label  # noqa: F401,E402  (src/imutils.py:477; the label CRF)
from .ir_label import cam_to_ir_label, combine_conf  # noqa: F401,E402  (IR labels from CAMs; script: muscle_amd.cam_to_ir_label)
from .lattice import PermutohedralLattice  # noqa: F401,E402  (the lattice filter; pairwise="lattice" of the CRFs)
from .crf_loss import DenseEnergyLoss  # noqa: F401,E402  (dense-CRF energy loss of decoder training; train_muscle --energy_weight)
from .lovasz import LovaszSoftmaxLoss, lovasz_softmax  # noqa: F401,E402  (Lovasz-softmax loss on label maps; train_muscle --lovasz_weight)
from .pamr import PAMR, pamr_affinity, pamr_apply  # noqa: F401,E402  (pixel-adaptive mask refinement; infer_mcl / infer_seg --pamr_iters)
from .ins_seg import (InstanceLabels, cluster_centroids, connected_components, find_centroids,  # noqa: F401,E402
                      infer_irn_instances)  # (instance pseudo-labels from the displacement field; infer_irn --ins_seg_out_dir)

_INS_EVAL = ("InsSegEval", "voc_instances", "pair_table", "mask_iou", "label_pair_counts", "mask_pair_counts")

_IRN_SWEEP = ("IrnSweep",)

# class-balanced self-training labels from infer_seg's confidences (script: muscle_amd.selflabel)
_SELFLABEL = ("conf_code", "ConfStats", "thresholds", "quality_curve", "select", "code_of", "code_interval")


def __getattr__(name):
    # instance-segmentation evaluation (script: muscle_amd.ins_eval).  Resolved on first use, so that `python -m muscle_amd.ins_eval`
    # does not find its own module imported by the package before it runs.
    if name in _INS_EVAL:
        from . import ins_eval
        return getattr(ins_eval, name)
    if name in _IRN_SWEEP:                       # the infer_irn grid sweep (script: muscle_amd.irn_sweep), resolved the same way
        from . import irn_sweep
        return getattr(irn_sweep, name)
    if name in _SELFLABEL:
        from . import selflabel
        return getattr(selflabel, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
