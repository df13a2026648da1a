"""`DeformableDETR`: the plain detector of configs/deformable_detr/od_r101_vg.py:3-96 and
od_rnext101_vg.py ([3P] mmdet `DeformableDETR(DETR(SingleStageDetector))`): backbone ->
ChannelMapper -> `DeformableDETRHead` (det_head.py).  Backbone / neck construction, `to()` and the
state-dict layout `backbone.* / neck.* / bbox_head.*` are `PSGTr`'s (detector.py), by inheritance;
what differs is the head table and the results: `simple_test` / `detect` return mmdet's
`bbox2result` lists, `val_det_losses` the detection loss values (det_losses.py)."""
import torch

from .det_head import DeformableDETRHead
from .detector import PSGTr


class DeformableDETR(PSGTr):
    @staticmethod
    def _head_types():
        return dict(DeformableDETRHead=DeformableDETRHead)

    def __init__(self, backbone, bbox_head, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, neck=None):
        bbox_head = dict(bbox_head)
        bbox_head.setdefault("type", "DeformableDETRHead")
        if neck is None:
            raise NotImplementedError("DeformableDETR: a ChannelMapper neck with 4 outputs "
                                      "(od_r101_vg.py:17-25)")
        super().__init__(backbone, bbox_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained, init_cfg=init_cfg, neck=neck)

    @torch.no_grad()
    def simple_test(self, img, img_metas, rescale=False):
        """mmdet `SingleStageDetector.simple_test`: one list per image of `num_classes` arrays
        [n_c, 5] (x1, y1, x2, y2, score)."""
        return self.bbox_head.simple_test(self.extract_feat(img), img_metas, rescale=rescale)

    @torch.no_grad()
    def detect(self, image, rescale=False):
        """Decoded uint8 (H, W, 3) BGR image (host or device) -> `simple_test`'s lists for that
        image: the od configs' test pipeline (vg_detection.py:27-43) on the GPU, then `simple_test`."""
        img, metas = self._pipeline_of_images()(image)
        return self.simple_test(img, metas, rescale=rescale)

    def _pipeline_of_images(self):
        """The od configs' own pipeline: pairnet.py's with Pad(size_divisor=32); set
        `self.test_pipeline` to a `preprocess.TestPipeline` to use another."""
        if self.test_pipeline is None:
            from .config import det_test_pipeline_cfg
            from .preprocess import TestPipeline
            self.test_pipeline = TestPipeline.from_config(det_test_pipeline_cfg(),
                                                          device=self.bbox_head.device)
        return self.test_pipeline

    @torch.no_grad()
    def val_det_losses(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, **kw):
        """The values mmdet's `forward_train` returns: extract_feat -> head forward (all decoder
        layers) -> `loss`: 3 * (L + 1) keys as 0-dim device tensors.  Forward only; keywords go to
        `DeformableDETRLoss.loss` (`grads={}`, `trace=[]`)."""
        metas = [dict(m) for m in img_metas]
        for m in metas:        # DETR.forward_train: batch_input_shape = the batch tensor's (H, W)
            m.setdefault("batch_input_shape", tuple(img.shape[-2:]))
        return self.bbox_head.val_det_losses(self.extract_feat(img), metas, gt_bboxes, gt_labels,
                                             gt_bboxes_ignore=gt_bboxes_ignore, **kw)

    def val_losses(self, *a, **kw):
        raise NotImplementedError("DeformableDETR: use val_det_losses(img, img_metas, gt_bboxes, "
                                  "gt_labels)")

    def forward_train(self, *a, **kw):
        return self.bbox_head.forward_train()
