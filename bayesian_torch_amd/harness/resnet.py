"""Deterministic ResNet skeletons that get fed to ``dnn_to_bnn``.

torchvision is not installed in this image, and the reference's README
(README.md:98-100) converts ``torchvision.models.resnet18()``.  This file is a
plain-PyTorch stand-in with the torchvision topology and *module names*
(``conv1, bn1, layer1.0.conv1, ..., layer4.1.bn2, fc``): 7x7/s2 stem, 3x3/s2
max-pool, four stages of residual blocks, adaptive average pool, one Linear.

It holds no Bayesian code at all -- the Bayesian layers are swapped in by
``bayesian_torch_amd.models.dnn_to_bnn.dnn_to_bnn`` exactly as the reference's
converter does for a user model (reference ``models/dnn_to_bnn.py:127-154``).

``width`` scales the channel counts (64 -> the standard model; 8 -> the tiny
model used for fully-stored golden fixtures).
"""
import torch
import torch.nn as nn


def _qact():
    from ..quantization import qact
    return qact


class _Basic(nn.Module):
    expansion = 1

    def __init__(self, cin, planes, stride, shortcut):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = shortcut

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        if getattr(self, "fused", False):          # fuse_inference(): bn/relu/add live in the conv kernels' output stage
            return self.conv2(self.conv1(x), residual=skip)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        if getattr(self, "u8", False):             # u8_inference(): y and skip are quint8 carriers, added as the reference's QResNet adds them
            return _qact().add_relu(y, skip)
        return self.relu(y + skip)

    def chain_members(self):
        """The fused forward above as a run of layers, each reading what the one before wrote -- what ``ResNet._run_stage`` may hand to
        ``FusedBayesLayer.forward_chain`` in this block's place: [(layer, residual)], residual None, "input" (the block's input) or the index
        of an earlier layer of the list. None when the block is not that: not fused, a shortcut that computes, u8 carriers, hooks on it."""
        if (not getattr(self, "fused", False) or self.downsample is not None or getattr(self, "u8", False) or self._forward_hooks
                or self._forward_pre_hooks):
            return None
        return [(self.conv1, None), (self.conv2, "input")]


class _Bottle(nn.Module):
    expansion = 4

    def __init__(self, cin, planes, stride, shortcut):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        # stride sits on the 3x3, as in reference models/deterministic/resnet_large.py:72-77
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = shortcut

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        if getattr(self, "fused", False):
            return self.conv3(self.conv2(self.conv1(x)), residual=skip)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        if getattr(self, "u8", False):
            return _qact().add_relu(y, skip)
        return self.relu(y + skip)


class ResNet(nn.Module):
    def __init__(self, block, depths, num_classes=10, width=64, in_ch=3):
        super().__init__()
        self._cin = width
        self.conv1 = nn.Conv2d(in_ch, width, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._stage(block, width, depths[0], 1)
        self.layer2 = self._stage(block, width * 2, depths[1], 2)
        self.layer3 = self._stage(block, width * 4, depths[2], 2)
        self.layer4 = self._stage(block, width * 8, depths[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(width * 8 * block.expansion, num_classes)

    def _stage(self, block, planes, n, stride):
        cout = planes * block.expansion
        shortcut = None
        if stride != 1 or self._cin != cout:
            shortcut = nn.Sequential(nn.Conv2d(self._cin, cout, 1, stride, bias=False),
                                     nn.BatchNorm2d(cout))
        mods = [block(self._cin, planes, stride, shortcut)]
        self._cin = cout
        mods += [block(cout, planes, 1, None) for _ in range(n - 1)]
        return nn.Sequential(*mods)

    @staticmethod
    def _run_stage(stage, x):
        """A stage of the fused model (fuse_inference). Consecutive blocks that describe themselves as a run of same-shape layers
        (``chain_members``: identity-shortcut basic blocks) go two blocks (four convs) at a time through
        ``FusedBayesLayer.forward_chain``: one launch where the shapes allow it (CIFAR-sized layer1). Anything else, and whatever the chain
        helper passes up (hooks on a member, gradients, no MC context, BT_CHAIN=0, shapes the library declines ...), runs block by block:
        the same results. Hooks on the stage, or registered for every module, see each call: then the stage runs as the Sequential it is."""
        from torch.nn.modules import module as _m
        from ..layers._fused import FusedBayesLayer
        if stage._forward_hooks or stage._forward_pre_hooks or _m._global_forward_hooks or _m._global_forward_pre_hooks:
            return stage(x)
        blocks, i = list(stage), 0
        while i < len(blocks):
            members, used = [], 0
            for b in blocks[i:i + 2]:
                desc = b.chain_members() if hasattr(b, "chain_members") else None
                if desc is None:
                    break
                base = len(members)      # the block's "input" is the run's input, or what the block before it wrote
                members += [(m, ("input" if base == 0 else base - 1) if r == "input" else r if r is None else base + r) for m, r in desc]
                used += 1
            if members:
                outs = FusedBayesLayer.forward_chain([m for m, _ in members], x, [r for _, r in members])
                if outs is not None:
                    x, i = outs[-1], i + used
                    continue
            x, i = blocks[i](x), i + 1
        return x

    def forward(self, x):
        if getattr(self, "fused", False):
            x = self.conv1(x)  # bn1 / relu / maxpool live in its output stage
            for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
                x = self._run_stage(stage, x)
        else:
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        if x.shape[-2:] != (1, 1):     # (CIFAR-sized inputs end on 1x1 maps: the mean of one element is that element -- no launch)
            x = self.avgpool(x)
        return self.fc(torch.flatten(x, 1))


def resnet18(num_classes=10, width=64):
    return ResNet(_Basic, [2, 2, 2, 2], num_classes, width)


def resnet50(num_classes=1000, width=64):
    return ResNet(_Bottle, [3, 4, 6, 3], num_classes, width)


def mlp(sizes=(3072, 512, 10)):
    """cfg2 of BASELINE.json: Linear -> ReLU -> Linear (...)."""
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i + 2 < len(sizes):
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


def bayes_layers(model):
    """Bayesian layers of a converted model, in ``named_modules`` order."""
    return [(n, m) for n, m in model.named_modules()
            if hasattr(m, "mu_kernel") or hasattr(m, "mu_weight")]


def fill_bayes_params(model, seed, mu_std=0.1, rho_mean=-3.0, rho_std=0.1):
    """Overwrite every (mu, rho) with a recipe that depends only on (seed, layer
    index, shape) -- so a reference-converted model and a model converted by this
    package get bit-identical parameters without sharing construction-time RNG.
    Same distribution as the layers' own init (reference linear_variational.py:137-138)."""
    with torch.no_grad():
        for i, (_, m) in enumerate(bayes_layers(model)):
            g = torch.Generator().manual_seed(seed * 1000 + i)
            for nm in ("mu_kernel", "rho_kernel", "mu_weight", "rho_weight", "mu_bias", "rho_bias"):
                p = getattr(m, nm, None)
                if p is None:
                    continue
                v = torch.randn(p.shape, generator=g)
                v = v * (mu_std if nm.startswith("mu") else rho_std) + (0.0 if nm.startswith("mu") else rho_mean)
                p.copy_(v.to(p.device))


def fuse_inference(model):
    """Fold every BatchNorm / ReLU / residual add of a converted ResNet into the Bayesian convs' output stage
    (bayesian_torch_amd.fuse).  The model must be converted (dnn_to_bnn), on its device and in eval()."""
    from ..fuse import fold_pair, fold_maxpool
    fold_pair(model.conv1, model.bn1, relu=True)
    fold_maxpool(model.conv1, model.maxpool)
    for stage in (model.layer1, model.layer2, model.layer3, model.layer4):
        for blk in stage:
            last = 3 if isinstance(blk, _Bottle) else 2
            for i in range(1, last + 1):
                fold_pair(getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}"), relu=True)   # the last ReLU runs after the fused add
            if blk.downsample is not None:
                fold_pair(blk.downsample[0], blk.downsample[1], relu=False)
                blk.downsample[1] = nn.Identity()
            blk.fused = True
    model.fused = True
    return model


def u8_inference(model):
    """Keep the activations of an INT8 ResNet u8 from the stem to the classifier (quantization/qact.py). The
    model must come from ``bnn_to_qbnn(fuse_conv_bn=True)`` (or ``quantization.convert(fuse_conv_bn=True)``): every conv quantised,
    every BatchNorm folded. The stem returns a quint8 carrier; ReLU, the max-pool, the average pool and flatten reach it through the
    model's own modules; every block ends in ``add_relu(y, skip)`` at the reference QResNet's scale, max(y.q_scale(), skip.q_scale())
    with zero point 0; ``fc`` dequantises."""
    from ..layers._quantized import _QuantizedLayer
    convs = [model.conv1]
    for stage in (model.layer1, model.layer2, model.layer3, model.layer4):
        for blk in stage:
            last = 3 if isinstance(blk, _Bottle) else 2
            convs += [getattr(blk, f"conv{i}") for i in range(1, last + 1)]
            bns = [getattr(blk, f"bn{i}") for i in range(1, last + 1)]
            if blk.downsample is not None:
                convs.append(blk.downsample[0])
                bns.append(blk.downsample[1])
            if not all(isinstance(b, nn.Identity) for b in bns):
                raise RuntimeError("u8_inference: an unfolded BatchNorm (convert with fuse_conv_bn=True): there is no quantised BatchNorm")
    if not isinstance(model.bn1, nn.Identity) or not all(isinstance(c, _QuantizedLayer) for c in convs) or not isinstance(model.fc, _QuantizedLayer):
        raise RuntimeError("u8_inference: the model must be converted by bnn_to_qbnn(fuse_conv_bn=True): every conv and the fc quantised, every BatchNorm folded")
    model.conv1.return_quantized = True
    for stage in (model.layer1, model.layer2, model.layer3, model.layer4):
        for blk in stage:
            blk.u8 = True
    model.u8 = True
    return model
