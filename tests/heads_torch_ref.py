"""The training losses of the distillation heads on the modules' own ``nn`` layers under torch autograd (fp32 on the module's
device, batch-statistics BatchNorm; MIOpen / rocBLAS kernels): the reference side of tests/test_gpu_conv_train.py and of the
timing tools.  Each function is the forward of the reference's module (models/hallucination_network.py, models/hrnet.py) written
with the layers that cmdiad_amd.models keeps as parameter containers; the package itself trains on cmdiad_amd/conv_train.py only."""
import torch
import torch.nn as nn

from cmdiad_amd.models.hallucination_network import feature_reshape, feature_reshape_back


def _device(module):
    return next(module.parameters()).device


def conv_ftof_losses(module, xyz, rgb, sigmoid):
    """HallucinationCrossModalityConv (hallucination_network.py:133-147) -> (distance_to_xyz_real, distance_to_rgb_real)."""
    dev = _device(module)
    xyz, rgb = xyz.to(dev).float(), rgb.to(dev).float()
    xyz_h = feature_reshape_back(module.rgb_conv(feature_reshape(rgb)))
    rgb_h = feature_reshape_back(module.xyz_conv(feature_reshape(xyz)))
    return module._losses(xyz_h, rgb_h, xyz, rgb, sigmoid)


def ftoi_mlp_loss(module, rgb_feature, xyz):
    """HallucinationRGBFeatureToXYZInputMLP (hallucination_network.py:174-182)."""
    dev = _device(module)
    rgb_feature = rgb_feature.reshape(rgb_feature.shape[0], rgb_feature.shape[1], -1)
    x = module.mlp(module.rgb_norm(rgb_feature.to(dev).float())).transpose(1, 2)
    h = nn.functional.interpolate(x.reshape(x.shape[0], x.shape[1], 56, 56), size=(224, 224), mode='bicubic')
    return module._mean_row_norm(h, xyz.to(dev), 1)


def ftoi_conv_loss(module, feature, img):
    """HallucinationFeatureToInputConv (hallucination_network.py:211-220)."""
    dev = _device(module)
    f = feature.to(dev).float().transpose(1, 2)
    h = module.conv1(f.reshape(f.shape[0], f.shape[1], 56, 56))
    h = nn.functional.interpolate(h, size=(224, 224), mode='bicubic')
    h = module.conv4(torch.relu(module.conv3(torch.relu(module.conv2(h)))))
    assert h.shape[1:] == (3, 224, 224) and img.shape[1:] == (3, 224, 224)
    return module._mean_row_norm(h, img.to(dev), 1)


def hrnet_loss(module, img, feature):
    """HRNet (hrnet.py:290-299): stem, layer1-3 through Bottleneck.forward, final_layer."""
    dev = _device(module)
    x = torch.relu(module.bn1(module.conv1(img.to(dev).float())))
    x = torch.relu(module.bn2(module.conv2(x)))
    x = module.final_layer(module.layer3(module.layer2(module.layer1(x))))
    assert tuple(x.shape[1:]) == (768, 56, 56) and tuple(feature.shape[1:]) == (3136, 768)
    return module._mean_row_norm(feature_reshape_back(x), feature.to(dev), 2)
