"""The HiFi-GAN generator restated from stock torch modules (nn.Conv1d, nn.ConvTranspose1d, weight_norm): the oracle of
tests/test_hifigan_cpu.py and tests/test_gpu_hifigan.py.  It is written from the definition in DESIGN.md section 7
("HiFi-GAN vocoder") and shares no code with forwardtacotron_amd/hifigan.py: the modules' own forward runs here, per
item, in float64 or fp32, with every stage's output kept.

Also here: the float64 restatement of each KERNEL's stage from given (fp32-rounded) inputs together with the a-priori
error bound of an fp32 fma chain, (K + 4) * 2^-24 * sum |w| |x| (K the contraction length), the same sum formed with
absolute values."""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

PAD_VALUE = -11.5129
U = 2.0 ** -24
V1 = dict(resblock='1', upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
          resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), num_mels=80)
V2 = dict(V1, upsample_initial_channel=128)
V3 = dict(resblock='2', upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8), upsample_initial_channel=256,
          resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12)), num_mels=80)
PRESETS = {'full': V1, 'narrow': V2, 'rb2': V3}


def _wn(m):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return nn.utils.weight_norm(m)


class RefResBlock1(nn.Module):
    def __init__(self, ch, k, dilation):
        super().__init__()
        self.convs1 = nn.ModuleList([_wn(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=d * (k - 1) // 2)) for d in dilation])
        self.convs2 = nn.ModuleList([_wn(nn.Conv1d(ch, ch, k, 1, dilation=1, padding=(k - 1) // 2)) for _ in dilation])

    def forward(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            xt = F.leaky_relu(x, 0.1)
            xt = c1(xt)
            xt = F.leaky_relu(xt, 0.1)
            xt = c2(xt)
            x = xt + x
        return x


class RefResBlock2(nn.Module):
    def __init__(self, ch, k, dilation):
        super().__init__()
        self.convs = nn.ModuleList([_wn(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=d * (k - 1) // 2)) for d in dilation])

    def forward(self, x):
        for c in self.convs:
            xt = F.leaky_relu(x, 0.1)
            xt = c(xt)
            x = xt + x
        return x


class RefGenerator(nn.Module):
    def __init__(self, resblock, upsample_rates, upsample_kernel_sizes, upsample_initial_channel, resblock_kernel_sizes,
                 resblock_dilation_sizes, num_mels=80):
        super().__init__()
        self.num_kernels = len(resblock_kernel_sizes)
        self.num_upsamples = len(upsample_rates)
        C0 = upsample_initial_channel
        self.conv_pre = _wn(nn.Conv1d(num_mels, C0, 7, 1, padding=3))
        block = RefResBlock1 if resblock == '1' else RefResBlock2
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            self.ups.append(_wn(nn.ConvTranspose1d(C0 // (2 ** i), C0 // (2 ** (i + 1)), k, u, padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = C0 // (2 ** (i + 1))
            for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(block(ch, k, d))
        self.conv_post = _wn(nn.Conv1d(ch, 1, 7, 1, padding=3))
        self.hop = 1
        for u in upsample_rates:
            self.hop *= u

    def forward(self, x):
        return self.stages(x)[2]

    def stages(self, mel):
        """mel [n_mels, T] or [B, n_mels, T] -> (the outputs of conv_pre and, per upsampling stage, of the transposed
        convolution and of the averaged residual blocks -- the order of HiFiGAN's 'stages'; the pre-tanh signal; the
        wav [B, 1, hop T]).  For a 2-D mel everything is returned without the batch dimension, the wav as [hop T]."""
        single = mel.dim() == 2
        x = mel.unsqueeze(0) if single else mel
        x = self.conv_pre(x)
        out = [x]
        for i in range(self.num_upsamples):
            x = F.leaky_relu(x, 0.1)
            x = self.ups[i](x)
            out.append(x)
            xs = None
            for j in range(self.num_kernels):
                if xs is None:
                    xs = self.resblocks[i * self.num_kernels + j](x)
                else:
                    xs += self.resblocks[i * self.num_kernels + j](x)
            x = xs / self.num_kernels
            out.append(x)
        x = F.leaky_relu(x)
        pre = self.conv_post(x)
        wav = torch.tanh(pre)
        if single:
            return [o[0] for o in out], pre[0, 0], wav[0, 0]
        return out, pre, wav


def build(seed, dtype=torch.float32, **cfg):
    """the stock tree under torch.manual_seed(seed), default initialisation, in eval mode"""
    torch.manual_seed(seed)
    return RefGenerator(**cfg).to(dtype).eval()


def int16_of(wav):
    """the published scale, our clamp, and the truncation"""
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


def _lrelu(x, slope=0.1):
    return F.leaky_relu(x, slope)


def conv_in_stage(mel, w, b):
    """mel fp32 [n_mels, T] -> (out [C, T], bound) in float64: K = 7 n_mels"""
    x = mel.double().unsqueeze(0)
    out = F.conv1d(x, w, b, padding=3)[0]
    mag = F.conv1d(x.abs(), w.abs(), b.abs(), padding=3)[0]
    return out, (7 * mel.shape[0] + 4) * U * mag


def upsample_stage(x, w, b, stride):
    """x fp32 [Cin, L] -> (out [Cout, stride L], bound): K = 2 Cin, the two taps of a phase"""
    a = _lrelu(x.double()).unsqueeze(0)
    out = F.conv_transpose1d(a, w, b, stride=stride, padding=stride // 2)[0]
    mag = F.conv_transpose1d(a.abs(), w.abs(), b.abs(), stride=stride, padding=stride // 2)[0]
    return out, (2 * x.shape[0] + 4) * U * mag


def resconv_stage(x, d, w, b, res=None, prev=None, nk=1, divide=False):
    """the residual convolution: x fp32 [C, L] -> (out, bound) in float64.  value = res + b + conv_{k, d}(lrelu(x)): K = k C,
    the residual inside the absolute sum, (k C + 4) u (sum |w| |x| + |res|).  With prev (the stage's running sum, fp32) the value
    is added to it, and with divide the sum is divided by nk: one rounding each of a result whose magnitude the absolute
    sum bounds -- the nk additions and the division of the average are spread over nk launches, one addition each."""
    C, k = x.shape[0], w.shape[2]
    a = _lrelu(x.double()).unsqueeze(0)
    pad = d * (k - 1) // 2
    out = F.conv1d(a, w, b, dilation=d, padding=pad)[0]
    mag = F.conv1d(a.abs(), w.abs(), b.abs(), dilation=d, padding=pad)[0]
    if res is not None:
        out, mag = out + res.double(), mag + res.double().abs()
    bound = (k * C + 4) * U * mag
    if prev is not None:
        out, mag = out + prev.double(), mag + prev.double().abs()
        bound = bound + U * mag
    if divide:
        out, mag, bound = out / nk, mag / nk, bound / nk
        bound = bound + U * mag
    return out, bound


def respair_stage(x, d, w1, b1, w2, b2, prev=None, nk=1, divide=False):
    """ResBlock1's pair: x fp32 [C, L] -> (out, bound).  The first convolution (K = k C) errs by at most e1 = (k C + 4) u
    sum |w| |x|; LeakyReLU is 1-Lipschitz, so the second (K = k C, the residual inside the absolute sum) carries |W2| e1 on
    top of its own (k C + 4) u (sum |w| |x| + |x|).  prev / divide as in resconv_stage."""
    C, k = x.shape[0], w1.shape[2]
    xd = x.double()
    a = _lrelu(xd).unsqueeze(0)
    p1, p2 = d * (k - 1) // 2, (k - 1) // 2
    mid = F.conv1d(a, w1, b1, dilation=d, padding=p1)
    e1 = (k * C + 4) * U * F.conv1d(a.abs(), w1.abs(), b1.abs(), dilation=d, padding=p1)
    h = _lrelu(mid)
    out = F.conv1d(h, w2, b2, padding=p2)[0] + xd
    mag = F.conv1d(h.abs(), w2.abs(), b2.abs(), padding=p2)[0] + xd.abs()
    bound = (k * C + 4) * U * mag + F.conv1d(e1, w2.abs(), padding=p2)[0]
    if prev is not None:
        out, mag = out + prev.double(), mag + prev.double().abs()
        bound = bound + U * mag
    if divide:
        out, mag, bound = out / nk, mag / nk, bound / nk
        bound = bound + U * mag
    return out, bound


def conv_out_stage(x, w, b):
    """x fp32 [C, L] -> (pre-tanh [L], bound [L]): K = 7 C.  tanh is 1-Lipschitz; its own rounding is added by the caller"""
    a = _lrelu(x.double(), 0.01).unsqueeze(0)
    pre = F.conv1d(a, w, b, padding=3)[0, 0]
    mag = F.conv1d(a.abs(), w.abs(), b.abs(), padding=3)[0, 0]
    return pre, (7 * x.shape[0] + 4) * U * mag
