"""Public names of the package (what a user of the reference looks for)."""
from .config import (ConfigDict, baseline_head_cfg, baseline_r50, bbox_head_cfg,  # noqa: F401
                     channel_mapper_cfg, cross_r101_vg, det_head_cfg, det_test_pipeline_cfg, det_train_cfg,
                     load_config,
                     od_r101_vg, od_rnext101_vg, pairnet_rnext101_vg,
                     pairnet_head_cfg, pairnet_r50, pairnet_swin, psgtr2_head_cfg, psgtr2_r50,
                     psgtr2_train_cfg,
                     swin_backbone_cfg, test_pipeline_cfg, train_pipeline_cfg)
from .psgtr_head2 import PSGTrHead2  # noqa: F401
from .backbone import ResNet50Hip, ResNeXtHip  # noqa: F401
from .swin import SwinTransformerHip  # noqa: F401
from .baseline_head import CrossHeadBaseline  # noqa: F401
from .bbox_head import CrossHeadBBox  # noqa: F401
from .neck import ChannelMapper  # noqa: F401
from .head import CrossHead2  # noqa: F401
from .pipeline import PipelinedHead  # noqa: F401
from .grad import (BackboneGrad, FfnDropout, HeadGrad, PixelDecoderGrad,  # noqa: F401
                   RelationTailGrad, SwinBackboneGrad, SwinStagesGrad, BBoxTailGrad)
from .seg_grad import (BaselineHeadGrad, PSGTr2HeadGrad, SegmenterHeadGrad,  # noqa: F401
                       SegPixelDecoderGrad)
from .train import TailTrainer  # noqa: F401
from .baseline_train import BaselineTrainer  # noqa: F401
from .bbox_train import BBoxTrainer  # noqa: F401
from .psgtr2_train import PSGTr2Trainer  # noqa: F401
from .bbox_losses import CrossHeadBBoxLoss  # noqa: F401
from .det_head import DeformableDETRHead  # noqa: F401
from .det_losses import DeformableDETRLoss  # noqa: F401
from .det_detector import DeformableDETR  # noqa: F401
from .seg_losses import Mask2FormerLoss  # noqa: F401
from .baseline_losses import BaselineRelationLoss  # noqa: F401
from .psgtr2_losses import PSGTrHead2Loss  # noqa: F401
from .preprocess import TestPipeline  # noqa: F401
from .train_pipeline import AugParams, HalfSizeMasks, TrainPipeline  # noqa: F401
from .detector import (PSGTr, Result, ResultStreamer, build_detector, load_checkpoint,  # noqa: F401
                       triplet2Result)
from .dist import all_gather_triplets, shard_indices  # noqa: F401
from .evaluation import (PanopticQuality, SceneGraphMetrics, StreamingEvaluator,  # noqa: F401
                         TripletEvaluator)
from .runner import (EpochRunner, TrainLog, epoch_order, resume, save_checkpoint)  # noqa: F401
from . import dataset  # noqa: F401  (PSG ground truth: load_psg, ann_info, eval_ground_truth, ...)

__all__ = ["ConfigDict", "load_config", "pairnet_head_cfg", "pairnet_r50", "CrossHead2",
           "PSGTr", "Result", "ResultStreamer", "build_detector", "load_checkpoint", "triplet2Result", "all_gather_triplets",
           "shard_indices", "PipelinedHead", "CrossHeadBaseline", "baseline_head_cfg",
           "baseline_r50", "PSGTrHead2", "psgtr2_head_cfg", "psgtr2_r50", "ResNet50Hip",
           "SwinTransformerHip", "pairnet_swin", "swin_backbone_cfg", "TestPipeline", "test_pipeline_cfg",
           "CrossHeadBBox", "ChannelMapper", "bbox_head_cfg", "channel_mapper_cfg", "cross_r101_vg",
           "TripletEvaluator", "SceneGraphMetrics", "StreamingEvaluator", "PanopticQuality", "dataset", "RelationTailGrad", "HeadGrad", "PixelDecoderGrad", "BackboneGrad", "SwinBackboneGrad", "SwinStagesGrad", "SegmenterHeadGrad", "BaselineHeadGrad", "SegPixelDecoderGrad", "TailTrainer", "BaselineTrainer", "FfnDropout",
           "TrainPipeline", "AugParams", "HalfSizeMasks", "train_pipeline_cfg", "Mask2FormerLoss",
           "BaselineRelationLoss", "BBoxTailGrad", "BBoxTrainer", "CrossHeadBBoxLoss",
           "PSGTrHead2Loss", "psgtr2_train_cfg", "PSGTr2HeadGrad", "PSGTr2Trainer",
           "ResNeXtHip", "pairnet_rnext101_vg",
           "DeformableDETR", "DeformableDETRHead", "DeformableDETRLoss", "od_r101_vg",
           "od_rnext101_vg", "det_head_cfg", "det_train_cfg", "det_test_pipeline_cfg",
           "EpochRunner", "TrainLog", "epoch_order", "resume", "save_checkpoint"]
