"""Leaf-evaluation network: plumbing around the reference's `NNArch` weights.

* `NetSpec` / `LeafNet` restate the inference forward of the reference's `NNArch`
  (/root/reference/src/neural_net.py:211-230 DenseBlock, :233-263 ResidualBlock, :266-510 NNArch) with
  IDENTICAL parameter names, so a reference checkpoint's `state_dict` loads unchanged and a
  random-init net of the same architecture can be built without the reference tree.
* `process()` mirrors `NNWrapper.process` (neural_net.py:800-823): eval mode, optional bf16
  autocast, returns `exp(log_softmax)` as float32 probabilities.
* `fold()` folds inference BatchNorms into the convolutions and lays the weights out for the
  hand-written MFMA kernels in csrc/ (see DESIGN.md §Leaf net).

Covered: both trunks - the ResNet one (`dense_net=False`, what BASELINE.json's configs use) and the DenseNet one
(`dense_net=True`, the reference's `TrainConfig` default: no stem, `conv_layers.{i}` = DenseBlock with bn_size 4) - with
`trunk_norm` "batch" or "layer" (`nn.GroupNorm(1, C)`: per-sample statistics over (C, H, W); the heads keep BatchNorm),
`trunk_act` "relu" or "crelu" (`cat([relu(x), relu(-x)])`: the convolution behind it has twice the input channels), any odd
`kernel_size` in 1..7 (the HIP tiers: 3, and 1 / 5 / 7 on dense trunks), the value head, the flat policy head with or without
its FC stack (`pi_fc_layers`: pi_fc1 - ReLU - pi_fc_extra - pi_fc_out) and the spatial policy head.  The eight norm x activation x
trunk combinations all run on the fp32 tier (csrc/leafnet_f32.hip); of the matrix-core tiles the dense Connect4 one also takes
`trunk_norm="layer"` (csrc/leafnet_dense.h), the others keep batch / relu / no FC stack.  A dense trunk has two bf16 tiles: the
Connect4 family (6x7, flat policy head) and the spatial-head family on 7x7 / 11x11 / 13x13 (csrc/leafnet_dense_sp.h:
`stargambit_dense_spec()` on the unified canvas, `stargambit_variant_dense_spec(v)` in the four single-variant games' own shapes).
NOT covered: `head_pool=False` builds in torch but no HIP tier takes it; a spatial head has no FC stack (the reference's
`spatial_policy="auto"` falls back to the flat head then: here the caller leaves `policy_shape` out).
"""
from dataclasses import dataclass

import torch
import torch.nn as nn


@dataclass
class NetSpec:
    in_shape: tuple          # CANONICAL_SHAPE (C, H, W)
    num_moves: int
    num_players: int
    num_channels: int = 64   # NNArgs.num_channels
    depth: int = 6           # NNArgs.depth
    kernel_size: int = 3
    head_channels: int = 32
    head_pool: bool = True
    v_fc_hidden: int = -1    # -1 -> head_channels * 8 (neural_net.py:92-95)
    v_head_convs: int = 0
    pi_head_convs: int = 0
    v_fc_layers: int = 1
    policy_shape: tuple = None  # POLICY_SHAPE (C, H, W) -> spatial head (neural_net.py:390-427)
    pi_fc_hidden: int = -1   # -1 -> head_channels * 8; hidden width of pi_global (spatial head with global actions)
    dense_net: bool = False  # NNArgs.dense_net: DenseNet trunk, num_channels = the growth rate (neural_net.py:302-338)
    trunk_norm: str = "batch"   # NNArgs.trunk_norm: "batch" or "layer" = GroupNorm(1, C) on every trunk norm (neural_net.py:166-180)
    trunk_act: str = "relu"     # NNArgs.trunk_act: "relu" or "crelu" (neural_net.py:183-208)
    pi_fc_layers: int = 0       # NNArgs.pi_fc_layers: hidden layers (width pi_fc_hidden) of the flat policy head (neural_net.py:431-442)

    def __post_init__(self):
        if self.kernel_size not in (1, 3, 5, 7):
            raise ValueError("kernel_size must be an odd value in 1..7")
        if self.trunk_norm not in ("batch", "layer"):
            raise ValueError(f"trunk_norm must be 'batch' or 'layer', got {self.trunk_norm!r}")
        if self.trunk_act not in ("relu", "crelu"):
            raise ValueError(f"trunk_act must be 'relu' or 'crelu', got {self.trunk_act!r}")
        if self.pi_fc_layers < 0:
            raise ValueError("pi_fc_layers must be >= 0")
        if self.pi_fc_layers > 0 and self.policy_shape is not None:
            raise ValueError("pi_fc_layers > 0 is the flat policy head's FC stack: leave policy_shape out")
        if self.v_fc_hidden == -1:
            self.v_fc_hidden = self.head_channels * 8
        if self.pi_fc_hidden == -1:
            self.pi_fc_hidden = self.head_channels * 8


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding="same", bias=False)  # neural_net.py:147-155


def _norm(ch, kind):  # neural_net.py:166-180
    return nn.GroupNorm(1, ch) if kind == "layer" else nn.BatchNorm2d(ch)


class CReLU(nn.Module):  # neural_net.py:183-194
    def forward(self, x):
        return torch.cat([torch.relu(x), torch.relu(-x)], dim=1)


def _act(ch, kind):
    """(activation, channels behind it)  neural_net.py:197-208"""
    return (CReLU(), 2 * ch) if kind == "crelu" else (nn.ReLU(inplace=True), ch)


class ResidualBlock(nn.Module):  # neural_net.py:233-263 (no downsample)
    def __init__(self, ch, k, norm="batch", act="relu"):
        super().__init__()
        self.bn1 = _norm(ch, norm)
        self.relu1, c1 = _act(ch, act)
        self.conv1 = _conv(c1, ch, k)
        self.bn2 = _norm(ch, norm)
        self.relu2, c2 = _act(ch, act)
        self.conv2 = _conv(c2, ch, k)

    def forward(self, x):
        out = self.conv1(self.relu1(self.bn1(x)))
        out = self.conv2(self.relu2(self.bn2(out)))
        return out + x


class DenseBlock(nn.Module):  # neural_net.py:211-230
    def __init__(self, cin, growth, bn_size=4, k=3, norm="batch", act="relu"):
        super().__init__()
        self.bn1 = _norm(cin, norm)
        self.relu1, c1 = _act(cin, act)
        self.conv1 = _conv(c1, growth * bn_size, 1)
        self.bn2 = _norm(growth * bn_size, norm)
        self.relu2, c2 = _act(growth * bn_size, act)
        self.conv2 = _conv(c2, growth, k)

    def forward(self, x):
        out = self.conv1(self.relu1(self.bn1(x)))
        out = self.conv2(self.relu2(self.bn2(out)))
        return torch.cat([x, out], 1)


class LeafNet(nn.Module):
    def __init__(self, spec: NetSpec):
        super().__init__()
        self.spec = spec
        C, H, W = spec.in_shape
        ch, HC, k = spec.num_channels, spec.head_channels, spec.kernel_size
        norm, act = spec.trunk_norm, spec.trunk_act
        if spec.dense_net:   # no stem (neural_net.py:302-306); the heads read every feature (:332-335)
            self.conv_layers = nn.Sequential(*[DenseBlock(C + ch * i, ch, 4, k, norm, act) for i in range(spec.depth)])
            trunk_out = C + ch * spec.depth
        else:
            self.conv1 = _conv(C, ch, k)
            self.bn1 = _norm(ch, norm)
            self.conv_layers = nn.Sequential(*[ResidualBlock(ch, k, norm, act) for _ in range(spec.depth)])
            trunk_out = ch
        self.v_conv = _conv(trunk_out, HC, 1)
        self.pi_conv = _conv(trunk_out, HC, 1)
        self.v_bn = nn.BatchNorm2d(HC)
        self.v_relu = nn.ReLU(inplace=True)
        if spec.v_head_convs > 0:
            layers = []
            for _ in range(spec.v_head_convs):
                layers += [_conv(HC, HC, k), nn.BatchNorm2d(HC), nn.ReLU(inplace=True)]
            self.v_extra_convs = nn.Sequential(*layers)
        self.v_pool = nn.AdaptiveAvgPool2d(1) if spec.head_pool else None
        self.v_flatten = nn.Flatten()
        self.v_fc1 = nn.Linear(HC if spec.head_pool else HC * H * W, spec.v_fc_hidden)
        self.v_fc1_relu = nn.ReLU(inplace=True)
        if spec.v_fc_layers > 1:
            extra = []
            for _ in range(spec.v_fc_layers - 1):
                extra += [nn.Linear(spec.v_fc_hidden, spec.v_fc_hidden), nn.ReLU(inplace=True)]
            self.v_fc_extra = nn.Sequential(*extra)
        self.v_fc2 = nn.Linear(spec.v_fc_hidden, spec.num_players + 1)
        self.pi_bn = nn.BatchNorm2d(HC)
        self.pi_relu = nn.ReLU(inplace=True)
        if spec.pi_head_convs > 0:
            layers = []
            for _ in range(spec.pi_head_convs):
                layers += [_conv(HC, HC, k), nn.BatchNorm2d(HC), nn.ReLU(inplace=True)]
            self.pi_extra_convs = nn.Sequential(*layers)
        if spec.policy_shape is not None:
            pc, ph, pw = spec.policy_shape
            assert (ph, pw) == (H, W) and pc * ph * pw <= spec.num_moves
            self.pi_conv2 = _conv(HC, pc, 1)
            self.pi_bn2 = nn.BatchNorm2d(pc)
            self.num_global_actions = spec.num_moves - pc * ph * pw
            if self.num_global_actions > 0:   # neural_net.py:413-426: deploys + end turn of StarGambit
                self.pi_flatten = nn.Flatten()
                self.pi_pool = nn.AdaptiveAvgPool2d(1) if spec.head_pool else None
                self.pi_global = nn.Sequential(nn.Linear(HC if spec.head_pool else HC * H * W, spec.pi_fc_hidden), nn.ReLU(inplace=True),
                                               nn.Linear(spec.pi_fc_hidden, self.num_global_actions), nn.LayerNorm(self.num_global_actions))
        else:
            self.pi_flatten = nn.Flatten()
            if spec.pi_fc_layers > 0:   # neural_net.py:431-442
                self.pi_fc1 = nn.Linear(H * W * HC, spec.pi_fc_hidden)
                if spec.pi_fc_layers > 1:
                    extra = []
                    for _ in range(spec.pi_fc_layers - 1):
                        extra += [nn.Linear(spec.pi_fc_hidden, spec.pi_fc_hidden), nn.ReLU(inplace=True)]
                    self.pi_fc_extra = nn.Sequential(*extra)
                self.pi_fc_out = nn.Linear(spec.pi_fc_hidden, spec.num_moves)
            else:
                self.pi_fc1 = nn.Linear(H * W * HC, spec.num_moves)

    def forward(self, s):  # neural_net.py:448-510 — returns LOG-probabilities like the reference
        if not self.spec.dense_net:
            s = self.bn1(self.conv1(s))
        s = self.conv_layers(s)
        v = self.v_relu(self.v_bn(self.v_conv(s)))
        if hasattr(self, "v_extra_convs"):
            v = self.v_extra_convs(v)
        if self.v_pool is not None:
            v = self.v_pool(v)
        v = self.v_fc1_relu(self.v_fc1(self.v_flatten(v)))
        if hasattr(self, "v_fc_extra"):
            v = self.v_fc_extra(v)
        v = torch.log_softmax(self.v_fc2(v), dim=1)
        pi = self.pi_relu(self.pi_bn(self.pi_conv(s)))
        if hasattr(self, "pi_extra_convs"):
            pi = self.pi_extra_convs(pi)
        if self.spec.policy_shape is not None:
            sp = self.pi_bn2(self.pi_conv2(pi)).permute(0, 2, 3, 1).reshape(pi.shape[0], -1)
            if self.num_global_actions > 0:   # neural_net.py:486-493
                flat = self.pi_flatten(self.pi_pool(pi) if self.pi_pool is not None else pi)
                sp = torch.cat([sp, self.pi_global(flat)], dim=1)
            pi = sp
        elif self.spec.pi_fc_layers > 0:   # neural_net.py:497-504
            pi = torch.relu(self.pi_fc1(self.pi_flatten(pi)))
            if hasattr(self, "pi_fc_extra"):
                pi = self.pi_fc_extra(pi)
            pi = self.pi_fc_out(pi)
        else:
            pi = self.pi_fc1(self.pi_flatten(pi))
        return v, torch.log_softmax(pi, dim=1)

    @torch.no_grad()
    def process(self, batch, amp_dtype=None):
        """NNWrapper.process (neural_net.py:800-823): probabilities as float32."""
        self.eval()
        if amp_dtype is not None:
            with torch.amp.autocast(batch.device.type, dtype=amp_dtype):
                v, pi = self(batch)
        else:
            v, pi = self(batch)
        return torch.exp(v).float(), torch.exp(pi).float()


def connect4_spec(depth=6, channels=64, kernel_size=3, head_channels=32):
    """BASELINE config 2: Connect4, 6 blocks x 64 channels, k=3, flat policy head."""
    return NetSpec(in_shape=(4, 6, 7), num_moves=7, num_players=2, num_channels=channels, depth=depth,
                   kernel_size=kernel_size, head_channels=head_channels)


def connect4_dense_spec(depth=4, channels=12, kernel_size=5, head_channels=32):
    """The reference's TrainConfig defaults (config.py:44-60; Connect4 has no YAML): DenseNet trunk, growth 12, 4 blocks, k=5."""
    return NetSpec(in_shape=(4, 6, 7), num_moves=7, num_players=2, num_channels=channels, depth=depth,
                   kernel_size=kernel_size, head_channels=head_channels, dense_net=True)


def stargambit_dense_spec(depth=4, channels=16, kernel_size=3, head_channels=32):
    """configs/star_gambit_skirmish.yaml and its single-variant siblings: they set kernel_size 3 and inherit the dense default;
    spatial head over the 13 x 13 canvas + 19 global actions."""
    return NetSpec(in_shape=(36, 13, 13), num_moves=1709, num_players=2, num_channels=channels, depth=depth,
                   kernel_size=kernel_size, head_channels=head_channels, policy_shape=(10, 13, 13), dense_net=True)


def stargambit_variant_dense_spec(variant, depth=4, channels=16, kernel_size=3, head_channels=32):
    """configs/star_gambit_{skirmish,showdown,clash,battle}.yaml (variant 0..3) in the game's OWN shapes
    (games.StarGambit{Skirmish,Showdown,Clash,Battle}GS): 32 planes on 11 x 11 (variants 0-2) or 13 x 13 (Battle), the dense
    default, spatial head with 10 channels + 19 global actions."""
    if variant not in (0, 1, 2, 3):
        raise ValueError("variant must be 0 (Skirmish), 1 (Showdown), 2 (Clash) or 3 (Battle)")
    d = 13 if variant == 3 else 11
    return NetSpec(in_shape=(32, d, d), num_moves=10 * d * d + 19, num_players=2, num_channels=channels, depth=depth,
                   kernel_size=kernel_size, head_channels=head_channels, policy_shape=(10, d, d), dense_net=True)


def tawlbwrdd_spec(depth=4):
    """BASELINE config 3 / configs/tawlbwrdd.yaml:6-16: 4 blocks x 64 channels, k=3, head_channels 64,
    one extra conv per head, two value FC layers, spatial policy head (POLICY_SHAPE 22 x 11 x 11)."""
    return NetSpec(in_shape=(7, 11, 11), num_moves=2662, num_players=2, num_channels=64, depth=depth, kernel_size=3,
                   head_channels=64, v_head_convs=1, pi_head_convs=1, v_fc_layers=2, policy_shape=(22, 11, 11))


def brandubh_spec():
    """configs/brandubh.yaml: 4 blocks x 32 channels, head_channels 32, extra head convs, two value FC layers, spatial head."""
    return NetSpec(in_shape=(7, 7, 7), num_moves=686, num_players=2, num_channels=32, depth=4, kernel_size=3, head_channels=32,
                   v_head_convs=1, pi_head_convs=1, v_fc_layers=2, policy_shape=(14, 7, 7))


def opentafl_spec(depth=4, channels=64, head_channels=64):
    """OpenTafl: 8 canonical planes (plane 7 = turn / max_turns), 11x11, spatial head (the Tawlbwrdd YAML shape)."""
    return NetSpec(in_shape=(8, 11, 11), num_moves=2662, num_players=2, num_channels=channels, depth=depth, kernel_size=3,
                   head_channels=head_channels, v_head_convs=1, pi_head_convs=1, v_fc_layers=2, policy_shape=(22, 11, 11))


def stargambit_spec(depth=4, channels=64, head_channels=64):
    """BASELINE config 5 / configs/star_gambit_unified.yaml:5-15: 4 blocks x 64 channels, k=3, head_channels 64, one extra conv
    per head, two value FC layers, spatial policy head (POLICY_SHAPE 10 x 13 x 13) + 19 global actions (deploys, end turn)."""
    return NetSpec(in_shape=(36, 13, 13), num_moves=1709, num_players=2, num_channels=channels, depth=depth, kernel_size=3,
                   head_channels=head_channels, v_head_convs=1, pi_head_convs=1, v_fc_layers=2, policy_shape=(10, 13, 13))


def random_init(spec, seed=0, randomize_bn=True):
    """Random-init net of the named architecture (no checkpoint / dataset is reachable here).
    BatchNorm statistics and affine parameters are randomised too so that BN folding is exercised, and the trunk's
    GroupNorm weights and biases (trunk_norm="layer") in the same way: an identity affine hides a dropped one."""
    torch.manual_seed(seed)
    net = LeafNet(spec)
    if randomize_bn:
        g = torch.Generator().manual_seed(seed + 1)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.0 + 0.5)
                m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.8 + 0.6)
                m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            elif isinstance(m, nn.GroupNorm):
                m.weight.data.copy_(torch.rand(m.num_channels, generator=g) * 0.8 + 0.6)
                m.bias.data.copy_(torch.randn(m.num_channels, generator=g) * 0.1)
    return net.eval()


def bn_affine(bn):
    """Inference BatchNorm as y = a * x + b."""
    a = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * a
    return a, b
