"""The MelGAN generator restated from stock torch modules (nn.Conv1d, nn.ConvTranspose1d, nn.ReflectionPad1d,
weight_norm): the oracle of tests/test_melgan_cpu.py and tests/test_gpu_melgan.py.  It is written from the definition in
DESIGN.md section 7 ("MelGAN vocoder") and shares no code with forwardtacotron_amd/melgan.py: the modules' own forward
runs here, per item, in float64 or fp32, with every stage's output kept.

Also here: the float64 restatement of each KERNEL's stage from given (fp32-rounded) inputs together with the a-priori
error bound of an fp32 fma chain, (K + 4) * 2^-24 * sum |w| |x| (K the contraction length), the same sum formed with
absolute values."""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

PAD_VALUE = -11.5129
U = 2.0 ** -24
FULL = dict(mel_channel=80, channels=(512, 256, 128, 64, 32), upsamples=((16, 8, 4), (16, 8, 4), (4, 2, 1), (4, 2, 1)))
NARROW = dict(mel_channel=8, channels=(32, 16, 16, 8, 8), upsamples=((16, 8, 4), (16, 8, 4), (4, 2, 1), (4, 2, 1)))


def _wn(m):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return nn.utils.weight_norm(m)


class RefResStack(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.blocks = nn.ModuleList([
            nn.Sequential(nn.LeakyReLU(0.2), nn.ReflectionPad1d(3 ** i),
                          _wn(nn.Conv1d(channel, channel, kernel_size=3, dilation=3 ** i)),
                          nn.LeakyReLU(0.2), _wn(nn.Conv1d(channel, channel, kernel_size=1)))
            for i in range(3)])
        self.shortcuts = nn.ModuleList([_wn(nn.Conv1d(channel, channel, kernel_size=1)) for i in range(3)])

    def forward(self, x):
        for block, shortcut in zip(self.blocks, self.shortcuts):
            x = shortcut(x) + block(x)
        return x


class RefGenerator(nn.Module):
    def __init__(self, mel_channel=80, channels=(512, 256, 128, 64, 32),
                 upsamples=((16, 8, 4), (16, 8, 4), (4, 2, 1), (4, 2, 1))):
        super().__init__()
        layers = [nn.ReflectionPad1d(3), _wn(nn.Conv1d(mel_channel, channels[0], kernel_size=7, stride=1))]
        for i, (k, s, p) in enumerate(upsamples):
            layers += [nn.LeakyReLU(0.2),
                       _wn(nn.ConvTranspose1d(channels[i], channels[i + 1], kernel_size=k, stride=s, padding=p)),
                       RefResStack(channels[i + 1])]
        layers += [nn.LeakyReLU(0.2), nn.ReflectionPad1d(3), _wn(nn.Conv1d(channels[4], 1, kernel_size=7, stride=1)),
                   nn.Tanh()]
        self.generator = nn.Sequential(*layers)
        self.hop = 1
        for _, s, _ in upsamples:
            self.hop *= s

    def forward(self, mel):
        return self.generator((mel + 5.0) / 5.0)

    def inference(self, mel):
        """mel [1, n_mels, T] -> int16 [hop * T]"""
        zero = torch.full((1, mel.shape[1], 10), PAD_VALUE, dtype=mel.dtype)
        audio = self.forward(torch.cat((mel, zero), dim=2)).squeeze()
        audio = audio[:-(self.hop * 10)]
        audio = 32768.0 * audio
        return audio.clamp(min=-32768.0, max=32768.0 - 1).short()

    def stages(self, mel, tail=10):
        """mel [n_mels, T] -> every stage's output [C, L] in the order of MelGAN._generate's kernels (input convolution;
        per upsampling stage the transposed convolution and the three residual blocks), then the pre-tanh signal [L]
        and the cut float wav [hop * T]"""
        g = self.generator
        x = mel.unsqueeze(0)
        if tail:
            x = torch.cat((x, torch.full((1, mel.shape[0], tail), PAD_VALUE, dtype=mel.dtype)), dim=2)
        x = g[1](g[0]((x + 5.0) / 5.0))
        out = [x[0]]
        for i in range(4):
            x = g[3 * i + 3](g[3 * i + 2](x))
            out.append(x[0])
            stack = g[3 * i + 4]
            for block, shortcut in zip(stack.blocks, stack.shortcuts):
                x = shortcut(x) + block(x)
                out.append(x[0])
        pre = g[16](g[15](g[14](x)))[0, 0]
        wav = torch.tanh(pre)
        return out, pre, wav[:self.hop * mel.shape[1]]


def build(seed, dtype=torch.float32, **cfg):
    """the stock tree under torch.manual_seed(seed), default initialisation, in eval mode"""
    torch.manual_seed(seed)
    return RefGenerator(**cfg).to(dtype).eval()


def int16_of(wav):
    """the reference's scale, clamp and truncate"""
    return (32768.0 * wav).clamp(min=-32768.0, max=32767.0).short()


def make_mels(lens, n_mels, seed, Tmax=None, pad=PAD_VALUE):
    """a padded fp32 batch [B, n_mels, Tmax] of log-mel-like values (in the reference's range, -11.5 .. 1) and the items"""
    gen = torch.Generator().manual_seed(seed)
    Tmax = Tmax or max(lens)
    mel = torch.full((len(lens), n_mels, Tmax), pad, dtype=torch.float32)
    items = []
    for b, n in enumerate(lens):
        m = (-5.0 + 2.5 * torch.randn(n_mels, n, generator=gen)).clamp(PAD_VALUE, 1.0)
        mel[b, :, :n] = m
        items.append(m)
    return mel, items


# ---- the float64 restatement of each kernel's stage with its a-priori bound -----------------------------------------
def folded(conv):
    """the weight-normed module's effective weight and bias in float64"""
    w = torch._weight_norm(conv.weight_v.detach().double(), conv.weight_g.detach().double(), 0)
    return w, conv.bias.detach().double()


def _lrelu(x):
    return F.leaky_relu(x, 0.2)


def _reflect(x, p):
    return F.pad(x.unsqueeze(0), (p, p), mode='reflect')[0]


def conv_in_stage(mel, tail, w, b):
    """mel fp32 [n_mels, T] -> (out [C, T + tail], bound) in float64: K = 7 n_mels"""
    x = mel.double()
    if tail:
        x = torch.cat((x, torch.full((x.shape[0], tail), float(torch.tensor(PAD_VALUE, dtype=torch.float32)),
                                     dtype=torch.float64)), dim=1)
    x = _reflect((x + 5.0) / 5.0, 3)
    out = F.conv1d(x.unsqueeze(0), w, b)[0]
    mag = F.conv1d(x.abs().unsqueeze(0), w.abs(), b.abs())[0]
    return out, (7 * mel.shape[0] + 4) * U * mag


def upsample_stage(x, w, b, stride):
    """x fp32 [Cin, L] -> (out [Cout, stride L], bound): K = 2 Cin, the two taps of a phase"""
    a = _lrelu(x.double()).unsqueeze(0)
    out = F.conv_transpose1d(a, w, b, stride=stride, padding=stride // 2)[0]
    mag = F.conv_transpose1d(a.abs(), w.abs(), b.abs(), stride=stride, padding=stride // 2)[0]
    return out, (2 * x.shape[0] + 4) * U * mag


def resblock_stage(x, d, w1, b1, w2, b2, ws, bs):
    """x fp32 [C, L] -> (out [C, L], bound).  The first convolution (K = 3 C) errs by at most e1 = (3 C + 4) u sum|w||x|;
    LeakyReLU is 1-Lipschitz, so the second product (K = 2 C: the 1x1 convolution and the shortcut in one accumulator)
    carries |W2| e1 on top of its own (2 C + 4) u sum|w||x|."""
    C = x.shape[0]
    x = x.double()
    a = _reflect(_lrelu(x), d).unsqueeze(0)
    mid = F.conv1d(a, w1, b1, dilation=d)
    e1 = (3 * C + 4) * U * F.conv1d(a.abs(), w1.abs(), b1.abs(), dilation=d)
    h = _lrelu(mid)
    out = F.conv1d(h, w2, b2) + F.conv1d(x.unsqueeze(0), ws, bs)
    mag = F.conv1d(h.abs(), w2.abs(), b2.abs()) + F.conv1d(x.abs().unsqueeze(0), ws.abs(), bs.abs())
    bound = (2 * C + 4) * U * mag + F.conv1d(e1, w2.abs())
    return out[0], bound[0]


def conv_out_stage(x, w, b):
    """x fp32 [C, L] -> (pre-tanh [L], bound [L]): K = 7 C.  tanh is 1-Lipschitz; its own rounding is added by the caller"""
    a = _reflect(_lrelu(x.double()), 3).unsqueeze(0)
    pre = F.conv1d(a, w, b)[0, 0]
    mag = F.conv1d(a.abs(), w.abs(), b.abs())[0, 0]
    return pre, (7 * x.shape[0] + 4) * U * mag
