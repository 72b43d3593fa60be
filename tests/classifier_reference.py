"""TEST INFRASTRUCTURE ONLY - the reference's Tortoise detector transcribed for the tests: AudioMiniEncoderWithClassifierHead as
tortoise/models/classifier.py builds it for api.classify_audio_clip, with arch_util's normalization / GroupNorm32 / Downsample /
AttentionBlock / QKVAttentionLegacy (no relative position bias), in plain torch.  Module names follow the reference, so the state_dict keys
are classifier.pth's."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def normalization(channels):
    groups = 32
    if channels <= 16:
        groups = 8
    elif channels <= 64:
        groups = 16
    while channels % groups != 0:
        groups = int(groups / 2)
    assert groups > 2
    return GroupNorm32(groups, channels)


class GroupNorm32(nn.GroupNorm):
    def forward(self, x):
        # the reference computes in (at least) f32; the fp64 transcription keeps fp64 here
        return super().forward(x if x.dtype == torch.float64 else x.float()).type(x.dtype)


class ResBlock(nn.Module):
    def __init__(self, channels, kernel_size=5):
        super().__init__()
        pad = 1 if kernel_size == 3 else 2
        self.in_layers = nn.Sequential(normalization(channels), nn.SiLU(), nn.Conv1d(channels, channels, kernel_size, padding=pad))
        self.out_layers = nn.Sequential(normalization(channels), nn.SiLU(), nn.Dropout(p=0.0),
                                        nn.Conv1d(channels, channels, kernel_size, padding=pad))

    def forward(self, x):
        return x + self.out_layers(self.in_layers(x))


class Downsample(nn.Module):
    def __init__(self, channels, out_channels, factor=4, ksize=5, pad=2):
        super().__init__()
        self.op = nn.Conv1d(channels, out_channels, ksize, stride=factor, padding=pad)

    def forward(self, x):
        return self.op(x)


class QKVAttentionLegacy(nn.Module):
    def __init__(self, n_heads):
        super().__init__()
        self.n_heads = n_heads

    def forward(self, qkv):
        bs, width, length = qkv.shape
        ch = width // (3 * self.n_heads)
        q, k, v = qkv.reshape(bs * self.n_heads, ch * 3, length).split(ch, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        weight = torch.einsum("bct,bcs->bts", q * scale, k * scale)
        weight = torch.softmax(weight.float(), dim=-1).type(weight.dtype)
        a = torch.einsum("bts,bcs->bct", weight, v)
        return a.reshape(bs, -1, length)


class AttentionBlock(nn.Module):
    def __init__(self, channels, num_heads):
        super().__init__()
        self.norm = normalization(channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.attention = QKVAttentionLegacy(num_heads)
        self.proj_out = nn.Conv1d(channels, channels, 1)

    def forward(self, x):
        return x + self.proj_out(self.attention(self.qkv(self.norm(x))))


class AudioMiniEncoder(nn.Module):
    def __init__(self, spec_dim=1, embedding_dim=512, base_channels=32, depth=5, resnet_blocks=2, attn_blocks=4, num_attn_heads=4,
                 downsample_factor=4, kernel_size=5):
        super().__init__()
        self.init = nn.Sequential(nn.Conv1d(spec_dim, base_channels, 3, padding=1))
        ch = base_channels
        res = []
        for _ in range(depth):
            for _ in range(resnet_blocks):
                res.append(ResBlock(ch, kernel_size))
            res.append(Downsample(ch, ch * 2, factor=downsample_factor))
            ch *= 2
        self.res = nn.Sequential(*res)
        self.final = nn.Sequential(normalization(ch), nn.SiLU(), nn.Conv1d(ch, embedding_dim, 1))
        self.attn = nn.Sequential(*[AttentionBlock(embedding_dim, num_attn_heads) for _ in range(attn_blocks)])
        self.dim = embedding_dim

    def forward(self, x):
        h = self.final(self.res(self.init(x)))
        h = self.attn(h)
        return h[:, :, 0]


class AudioMiniEncoderWithClassifierHead(nn.Module):
    def __init__(self, classes=2, **kwargs):
        super().__init__()
        self.enc = AudioMiniEncoder(**kwargs)
        self.head = nn.Linear(self.enc.dim, classes)

    def forward(self, x):
        return self.head(self.enc(x))


def build(sd=None, dtype=torch.float64):
    """The classifier api.classify_audio_clip builds, with `sd` loaded (or the torch default initialisation)."""
    m = AudioMiniEncoderWithClassifierHead(2)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dtype).eval()


@torch.no_grad()
def forward(model, clip):
    """clip [1, T] -> (logits [2], embedding [512]) in the model's dtype."""
    x = clip.to(next(model.parameters()).dtype).reshape(1, 1, -1)
    emb = model.enc(x)
    return model.head(emb)[0], emb[0]
