"""rroi_align.modules.rroi_align -- ``_RRoiAlign`` module.

Same constructor and call as ``rroi_align/modules/rroi_align.py:5-14`` of the
reference: ``_RRoiAlign(pooled_height, pooled_width, spatial_scale)(features, rois)``
with ``rois`` = ``(R, 6)`` rows ``[batch_idx, cx, cy, h, w, angle_deg]`` in
input-image pixels.  One optional keyword beyond the reference: ``channels_last_out=True`` returns
the crops in channels_last storage (same values) for a recognition head that runs in channels_last
-- MIOpen's preferred layout -- so that its first convolution does not relay 256 MiB out again;
the gradient that comes back in channels_last is consumed in place as well.  ``trig=1`` evaluates the
angle's cosine / sine with the device library's fp32 functions (what the reference's sources do when built
for this GPU) instead of the oracle's correctly rounded recipe; forward and backward of a call use the same.
``deterministic`` picks the backward's plan: ``None`` (default) follows ``torch.use_deterministic_algorithms`` as it
stands when the backward runs -- on: the ORDERED plan, the same gradient bits on every run (the oracle's double sum
in statement order, rounded once) --, ``True`` / ``False`` force the choice.

Precision: float32 features give float32 crops.  bfloat16 / float16 features (a model moved to that dtype, outside
torch.autocast) run natively: the crops and the feature gradient come back in the features' dtype, each element
computed in fp32 and rounded once -- the crops are bit for bit the fp32 op's crops of the widened features, rounded.
Under torch.autocast nothing changes: the features are cast up and the crops are float32.  ``rois`` are float32 always.
Channels_last 16-bit features and gradients are made contiguous before the call (no zero-copy form); channels_last
crops (``channels_last_out=True``) and a channels_last feature gradient are produced as for float32.
"""
from torch.nn.modules.module import Module

from ..functions.rroi_align import RRoiAlignFunction


class _RRoiAlign(Module):
    def __init__(self, pooled_height, pooled_width, spatial_scale, channels_last_out=False, trig=0,
                 deterministic=None):
        super(_RRoiAlign, self).__init__()
        self.deterministic = None if deterministic is None else bool(deterministic)
        self.trig = int(trig)   # 0 = TRIG_DOUBLE (default), 1 = TRIG_FP32: per call, see _ext.rroi_align
        self.pooled_width = int(pooled_width)
        self.pooled_height = int(pooled_height)
        self.spatial_scale = float(spatial_scale)
        self.channels_last_out = bool(channels_last_out)

    def forward(self, features, rois):
        return RRoiAlignFunction(self.pooled_height, self.pooled_width, self.spatial_scale,
                                 self.channels_last_out, self.trig, self.deterministic)(features, rois)

    def extra_repr(self):
        return "pooled_height={}, pooled_width={}, spatial_scale={}".format(
            self.pooled_height, self.pooled_width, self.spatial_scale)


class _RRoiAlignBucketed(Module):
    """RoIRotate with one pooled width PER ROI: ``_RRoiAlignBucketed(pooled_height, spatial_scale)(features, rois, widths)``
    -> ``[(index LongTensor (R_b,), crops (R_b, C, pooled_height, W_b))]`` in ascending width, the ROI order kept inside a
    bucket; ``widths`` is a host sequence of R ints.  Crop j of a bucket is bit for bit what
    ``_RRoiAlign(pooled_height, W_b, spatial_scale)(features, rois[index])[j]`` returns, but nothing wider is ever written
    and no bucket is sliced or copied out of a dense tensor: one launch chain for all widths, forward and backward.
    ``trig`` / ``deterministic`` and the dtype rules are ``_RRoiAlign``'s; features and crops are NCHW (channels_last
    features are made contiguous; their gradient comes back channels_last)."""

    def __init__(self, pooled_height, spatial_scale, trig=0, deterministic=None):
        super(_RRoiAlignBucketed, self).__init__()
        self.deterministic = None if deterministic is None else bool(deterministic)
        self.trig = int(trig)
        self.pooled_height = int(pooled_height)
        self.spatial_scale = float(spatial_scale)

    def forward(self, features, rois, widths):
        from ..functions.rroi_align import RRoiAlignBucketedFunction
        return RRoiAlignBucketedFunction(self.pooled_height, self.spatial_scale, self.trig, self.deterministic)(
            features, rois, widths)

    def extra_repr(self):
        return "pooled_height={}, spatial_scale={}".format(self.pooled_height, self.spatial_scale)
