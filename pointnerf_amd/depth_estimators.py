"""The pretrained depth estimator of the per-scene scripts (``manual_depth_view=1``, ``pre_d_est=.../MVSNet/model_000014.ckpt``) and the
2-D feature pyramid ``query_embedding`` samples: ``models/depth_estimators/mvsnet.py`` (``FeatureNet``, ``CostRegNet``, ``MVSNet``) with
``module.py``'s blocks, and ``models/mvs/models.py:717-764`` ``FeatureNet(intermediate=True)``.

The convolutions are plain torch modules in inference form (batch norm in eval): plumbing.  Their ``state_dict`` keys are the reference's, so
``model_000014.ckpt`` (after ``load_pretrained_d_est`` strips ``module.``) and ``*_net_mvs.pth`` load strictly.  Steps 2 and 3b-4 of
``MVSNet.forward`` -- the homography warp of every view with the variance over the views, and softmax + the two regressions + the padded
pool + gather -- are the two kernels of csrc/mvsdepth.hip (``ops.mvs_cost_volume``, ``ops.mvs_depth_regress``): no warped volume, no
probability volume unless it is returned.

``grid_sample`` in ``homo_warping`` (module.py:66) is called without ``align_corners``; under torch >= 1.3 -- every version the reference
supports -- that means ``align_corners=False``, although the normalisation two lines above it was written for ``True``.  The pretrained
weights are used with that half-pixel shift in all of the reference's runs, so it is the default here; ``MVSNet(align_corners=True)`` is the
geometry the normalisation was written for.

Training mode, enabled gradients and ``refine=True`` raise: the kernels have no backward, and the reference's ``RefineNet`` calls ``F.cat``,
which does not exist."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


# ---- models/depth_estimators/module.py:6-33 ----------------------------------------------------------------------------------------------
class ConvBnReLU(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class ConvBnReLU3D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = nn.BatchNorm3d(out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


# ---- models/depth_estimators/mvsnet.py:7-70 ----------------------------------------------------------------------------------------------
class FeatureNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.inplanes = 32
        self.conv0 = ConvBnReLU(3, 8, 3, 1, 1)
        self.conv1 = ConvBnReLU(8, 8, 3, 1, 1)
        self.conv2 = ConvBnReLU(8, 16, 5, 2, 2)
        self.conv3 = ConvBnReLU(16, 16, 3, 1, 1)
        self.conv4 = ConvBnReLU(16, 16, 3, 1, 1)
        self.conv5 = ConvBnReLU(16, 32, 5, 2, 2)
        self.conv6 = ConvBnReLU(32, 32, 3, 1, 1)
        self.feature = nn.Conv2d(32, 32, 3, 1, 1)

    def forward(self, x):
        x = self.conv1(self.conv0(x))
        x = self.conv4(self.conv3(self.conv2(x)))
        return self.feature(self.conv6(self.conv5(x)))


def _deconv3d(cin, cout):
    return nn.Sequential(nn.ConvTranspose3d(cin, cout, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False),
                         nn.BatchNorm3d(cout), nn.ReLU(inplace=True))


class CostRegNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv0 = ConvBnReLU3D(32, 8)
        self.conv1 = ConvBnReLU3D(8, 16, stride=2)
        self.conv2 = ConvBnReLU3D(16, 16)
        self.conv3 = ConvBnReLU3D(16, 32, stride=2)
        self.conv4 = ConvBnReLU3D(32, 32)
        self.conv5 = ConvBnReLU3D(32, 64, stride=2)
        self.conv6 = ConvBnReLU3D(64, 64)
        self.conv7 = _deconv3d(64, 32)
        self.conv9 = _deconv3d(32, 16)
        self.conv11 = _deconv3d(16, 8)
        self.prob = nn.Conv3d(8, 1, 3, stride=1, padding=1)

    def forward(self, x):
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


class MVSNet(nn.Module):
    """mvsnet.py:88-143 with ``refine=False``, inference only."""

    def __init__(self, refine=False, align_corners=False):
        super().__init__()
        if refine:
            raise NotImplementedError("MVSNet(refine=True): the reference's RefineNet calls F.cat, which does not exist (mvsnet.py:82); no "
                                      "script builds it")
        self.refine = refine
        self.align_corners = bool(align_corners)
        self.feature = FeatureNet()
        self.cost_regularization = CostRegNet()
        self.eval()

    def features_of(self, imgs):
        """step 1 on distinct images [V,3,H,W] -> [V,32,H/4,W/4]: one pass, whatever number of batch items share them"""
        return self.feature(imgs)

    def _cost_reg(self, imgs, proj_matrices, depth_values, features):
        """steps 1-3 (mvsnet.py:104-126) -> (the feature maps as one tensor, [V,32,h,w] when shared, else [B,V,32,h,w]; the logits [B,D,h,w])"""
        if self.training:
            raise NotImplementedError("MVSNet: training mode is not built (inference form only: batch norm in eval, kernels without a backward)")
        if torch.is_grad_enabled():
            raise NotImplementedError("MVSNet: gradients are enabled; call it under torch.no_grad() (the kernels have no backward)")
        ops._need_cuda(imgs, "imgs")
        if features is None:                                                          # step 1 (:106-107)
            features = [self.feature(imgs[:, v]) for v in range(imgs.shape[1])]
        stacked = features if isinstance(features, torch.Tensor) else torch.stack(list(features), dim=1)
        variance = ops.mvs_cost_volume(stacked, proj_matrices, depth_values, self.align_corners)      # step 2 (:110-122)
        return stacked, self.cost_regularization(variance).squeeze(1)                # step 3 (:125-126)

    def forward(self, imgs, proj_matrices, depth_values, features=None, prob_only=False):
        """imgs [B,V,3,H,W], proj_matrices [B,V,4,4], depth_values [B,D]; ``features``: the list over the views of [B,32,h,w] maps that
        the reference takes, or ONE tensor [V,32,h,w] that every batch item shares (what gen_points' expanded images amount to, :306).
        -> (depth [B,h,w], photometric_confidence [B,h,w], features, prob_volume [B,D,h,w]), or with ``prob_only`` (features, prob_volume,
        cost_reg)."""
        stacked, cost_reg = self._cost_reg(imgs, proj_matrices, depth_values, features)
        B, V = imgs.shape[:2]
        features = [stacked[v][None].expand(B, -1, -1, -1) if stacked.dim() == 4 else stacked[:, v] for v in range(V)]
        depth, confidence, prob_volume = ops.mvs_depth_regress(cost_reg, depth_values, return_prob=True)   # (:127-136)
        if prob_only:
            return features, prob_volume, cost_reg
        return depth, confidence, features, prob_volume

    def depth_and_confidence(self, imgs, proj_matrices, depth_values, features=None):
        """forward without the probability volume (gen_points drops it, models/mvs/mvs_points_model.py:314): nothing of size [B,D,h,w] is
        written besides the regulariser's own output"""
        return ops.mvs_depth_regress(self._cost_reg(imgs, proj_matrices, depth_values, features)[1], depth_values)


# ---- models/mvs/models.py:690-764: the 2-D pyramid of query_embedding ---------------------------------------------------------------------------
class ABN(nn.Module):
    """inplace_abn's ``InPlaceABN`` in inference form, restated: batch norm (eps 1e-5) followed by ``leaky_relu(0.01)``, its default
    activation.  Checkpoint keys ``weight, bias, running_mean, running_var``."""

    def __init__(self, num_features, eps=1e-5, slope=0.01):
        super().__init__()
        self.eps, self.slope = eps, slope
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def forward(self, x):
        if self.training:
            raise NotImplementedError("the 2-D feature pyramid is built in inference form only (batch statistics are not updated)")
        return F.leaky_relu(F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, False, 0.0, self.eps), self.slope)


class ConvABN(nn.Module):
    """models/mvs/models.py:690-701"""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = ABN(out_channels)

    def forward(self, x):
        return self.bn(self.conv(x))


class PyramidFeatureNet(nn.Module):
    """models/mvs/models.py:717-764 ``FeatureNet(intermediate=True)``: [B,V,3,H,W] -> [images [BV,3,H,W], [BV,8,H,W], [BV,16,H/2,W/2],
    [BV,32,H/4,W/4]]"""

    def __init__(self):
        super().__init__()
        self.conv0 = nn.Sequential(ConvABN(3, 8, 3, 1, 1), ConvABN(8, 8, 3, 1, 1))
        self.conv1 = nn.Sequential(ConvABN(8, 16, 5, 2, 2), ConvABN(16, 16, 3, 1, 1), ConvABN(16, 16, 3, 1, 1))
        self.conv2 = nn.Sequential(ConvABN(16, 32, 5, 2, 2), ConvABN(32, 32, 3, 1, 1), ConvABN(32, 32, 3, 1, 1))
        self.toplayer = nn.Conv2d(32, 32, 1)
        self.eval()

    def forward(self, x):
        B, V, _, H, W = x.shape
        x = x.reshape(B * V, 3, H, W)
        x1 = self.conv0(x)
        x2 = self.conv1(x1)
        x3 = self.toplayer(self.conv2(x2))
        return [x, x1, x2, x3]
