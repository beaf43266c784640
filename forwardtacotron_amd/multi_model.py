"""MI355X-native MultiForwardTacotron (speaker-embedding conditioned variant): drop-in for
models/multi_forward_tacotron.py:14-323 -- same constructor kwargs, batch-dict forward()/generate(), and
353-entry state_dict.  Built from the same HIP ops as forwardtacotron_amd.model plus the speaker concat,
the conditional predictors and the 3-class pitch_cond head.
"""
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn

from . import hip as H
from . import ops
from .base import AcousticModel, LengthRegulator, PAD_VALUE, predictor_front, predictor_tail
from .model import BatchNormConv, CBHG, ForwardTacotron, GRU, LSTM, conv_gru_predict, regulate_and_decode


class _SpeakerSeriesPredictor(nn.Module):
    """embedding ++ [pitch_cond embedding ++] speaker embedding -> 3 BatchNormConv -> biGRU -> Linear(out_dim): the two
    predictors below, which differ in the conditional embedding only"""

    def __init__(self, num_chars: int, emb_dim: int, conv_dims: int, rnn_dims: int, dropout: float,
                 speaker_emb_dims: int, out_dim: int = 1, cond_emb_size: int = 0, cond_emb_dims: int = 0):
        super().__init__()
        self.embedding = nn.Embedding(num_chars, emb_dim)
        if cond_emb_size:
            self.pitch_cond_embedding = nn.Embedding(cond_emb_size, cond_emb_dims)
        self.convs = nn.ModuleList([
            BatchNormConv(emb_dim + cond_emb_dims + speaker_emb_dims, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
            BatchNormConv(conv_dims, conv_dims, 5, relu=True),
        ])
        self.rnn = GRU(conv_dims, rnn_dims)
        self.lin = nn.Linear(2 * rnn_dims, out_dim)
        self.dropout = dropout

    def forward_lens(self, x: torch.Tensor, lens: torch.Tensor, semb: torch.Tensor, x_cond: Optional[torch.Tensor] = None,
                     alpha: float = 1.0) -> torch.Tensor:
        """eval forward of a ragged batch with one speaker row per item (semb [B,S]): tokens and x_cond at t >= lens[b]
        are ignored, the result [B,T,out_dim] is zero there.  The front stores zeros in the padding, speaker row
        included (the k = 5 convolutions would read it); x_cond: the conditional predictors."""
        B = x.shape[0]
        cond_w = self.pitch_cond_embedding.weight if x_cond is not None else None
        y = H.predictor_front_lens(x, lens, self.embedding.weight, x_cond, cond_w, semb)
        for conv in self.convs:
            y = conv.forward_lens(y, lens)
        y = self.rnn.forward_lens(y, lens, time_major_out=True)
        return H.mask_rows(predictor_tail(y, self.lin, alpha, B), lens)      # (the Linear's bias)


class SeriesPredictor(_SpeakerSeriesPredictor):
    """multi_forward_tacotron.py:14-50: embedding ++ speaker embedding -> 3 BatchNormConv -> biGRU -> Linear."""

    def __init__(self, num_chars: int, emb_dim: int = 64, conv_dims: int = 256, rnn_dims: int = 64,
                 dropout: float = 0.5, speaker_emb_dims: int = 256, out_dim: int = 1):
        super().__init__(num_chars, emb_dim, conv_dims, rnn_dims, dropout, speaker_emb_dims, out_dim)

    def forward(self, x: torch.Tensor, semb: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        return conv_gru_predict(self, predictor_front(x, self.embedding, speaker_emb=semb), alpha)


class ConditionalSeriesPredictor(_SpeakerSeriesPredictor):
    """multi_forward_tacotron.py:53-93: embedding ++ pitch_cond embedding ++ speaker embedding -> ..."""

    def __init__(self, num_chars: int, emb_dim: int = 64, cond_emb_size: int = 4, cond_emb_dims: int = 8,
                 conv_dims: int = 256, rnn_dims: int = 64, dropout: float = 0.5, speaker_emb_dims: int = 256):
        super().__init__(num_chars, emb_dim, conv_dims, rnn_dims, dropout, speaker_emb_dims,
                         cond_emb_size=cond_emb_size, cond_emb_dims=cond_emb_dims)

    def forward(self, x: torch.Tensor, x_cond: torch.Tensor, speaker_emb: torch.Tensor,
                alpha: float = 1.0) -> torch.Tensor:
        return conv_gru_predict(self, predictor_front(x, self.embedding, x_cond, self.pitch_cond_embedding, speaker_emb),
                                alpha)


class MultiForwardTacotron(AcousticModel):
    """Drop-in for models/multi_forward_tacotron.py:96-323."""
    config_key = 'multi_forward_tacotron'
    recurrent = True

    # Constructor keywords = the keys of config['multi_forward_tacotron']['model'] (+ num_chars, n_mels), exactly the
    # reference's (multi_forward_tacotron.py:98-129).
    _KEYS = ('embed_dims', 'series_embed_dims', 'num_chars', 'rnn_dims', 'n_mels', 'speaker_emb_dims',
             'pitch_cond_emb_dims', 'pitch_cond_categorical_dims', 'pitch_strength', 'energy_strength',
             'prenet_dims', 'prenet_k', 'prenet_num_highways', 'prenet_dropout',
             'postnet_dims', 'postnet_k', 'postnet_num_highways', 'postnet_dropout') + tuple(
        f'{p}_{k}' for p in ('durpred', 'pitch', 'pitch_cond', 'energy') for k in ('conv_dims', 'rnn_dims', 'dropout'))

    def __init__(self, padding_value=PAD_VALUE, **hp):
        super().__init__()
        missing = [k for k in self._KEYS if k not in hp]
        extra = [k for k in hp if k not in self._KEYS]
        if missing or extra:
            raise TypeError(f'MultiForwardTacotron(): missing {missing}, unexpected {extra}')
        self.rnn_dims = hp['rnn_dims']
        self.padding_value = padding_value
        self.speaker_emb_dims = hp['speaker_emb_dims']
        E, P, Q, S = hp['embed_dims'], hp['prenet_dims'], hp['postnet_dims'], hp['speaker_emb_dims']
        self.embedding = nn.Embedding(hp['num_chars'], E)
        self.lr = LengthRegulator()

        def predictor(kind, prefix, **more):
            # NB (reference quirk, multi_forward_tacotron.py:135-157): speaker_emb_dims is NOT forwarded to the
            # predictors, they keep their default of 256.
            return kind(num_chars=hp['num_chars'], emb_dim=hp['series_embed_dims'], conv_dims=hp[prefix + '_conv_dims'],
                        rnn_dims=hp[prefix + '_rnn_dims'], dropout=hp[prefix + '_dropout'], **more)

        # registration order = the reference's (it fixes the state_dict key order)
        self.dur_pred = predictor(ConditionalSeriesPredictor, 'durpred', cond_emb_dims=hp['pitch_cond_emb_dims'])
        self.pitch_cond_pred = predictor(SeriesPredictor, 'pitch_cond', out_dim=hp['pitch_cond_categorical_dims'])
        self.pitch_pred = predictor(ConditionalSeriesPredictor, 'pitch', cond_emb_dims=hp['pitch_cond_emb_dims'])
        self.energy_pred = predictor(SeriesPredictor, 'energy')
        self.prenet = CBHG(K=hp['prenet_k'], in_channels=E, channels=P, proj_channels=[P, E],
                           num_highways=hp['prenet_num_highways'], dropout=hp['prenet_dropout'])
        self.lstm = LSTM(2 * P + S, hp['rnn_dims'])
        self.lin = nn.Linear(2 * hp['rnn_dims'], hp['n_mels'])
        self.register_buffer('step', torch.zeros(1, dtype=torch.long))
        self.postnet = CBHG(K=hp['postnet_k'], in_channels=hp['n_mels'], channels=Q, proj_channels=[Q, hp['n_mels']],
                            num_highways=hp['postnet_num_highways'], dropout=hp['postnet_dropout'])
        self.post_proj = nn.Linear(2 * Q, hp['n_mels'], bias=False)
        self.pitch_strength = hp['pitch_strength']
        self.energy_strength = hp['energy_strength']
        self.pitch_proj = nn.Conv1d(1, 2 * P + S, kernel_size=3, padding=1)
        self.energy_proj = nn.Conv1d(1, 2 * P + S, kernel_size=3, padding=1)

    def _trunk(self, x, semb, dur, pitch, energy, mel_lens: Optional[torch.Tensor], late_inputs=None):
        """late_inputs (inference): delivers (dur, pitch, energy) once the prenet has been enqueued (see
        model.ForwardTacotron._trunk: the predictors run beside the prenet on the side stream)"""
        B, Tx = x.shape
        x = ops.EmbeddingFn.apply(x, self.embedding.weight)
        x = self.prenet(x, time_major_out=True)                                  # [Tx,B,2P]
        if late_inputs is not None:
            dur, pitch, energy = late_inputs()
        x = ops.ConcatColsFn.apply(x, None, semb, B, Tx, True)                   # [B,Tx,2P+S]
        x = ops.CondAddFn.apply(x, pitch, energy, self.pitch_proj.weight, self.pitch_proj.bias,
                                self.energy_proj.weight, self.energy_proj.bias, self.pitch_strength,
                                self.energy_strength, False)
        x = regulate_and_decode(self, x, dur, mel_lens)
        mel = ops.LinearFn.apply(x, self.lin.weight, self.lin.bias)
        post = self.postnet(mel, time_major_out=True)
        post = ops.LinearFn.apply(post, self.post_proj.weight, None, B)
        return mel, post

    def _predict(self, x, semb, pitch_cond=None, alpha: float = 1.0, pitch_function=lambda p: p,
                 energy_function=lambda e: e):
        """the four predictors, in the order that fixes the dropout seed sequence: pitch_cond, dur, pitch, energy.
        pitch_cond None (generate): the argmax of the pitch_cond predictor conditions the other two -- a chain that
        only works for B = 1, like the reference's (multi_forward_tacotron.py:258-262)"""
        pitch_cond_hat = self.pitch_cond_pred(x, semb).squeeze(-1)               # [B,Tx,3]
        if pitch_cond is None:
            pitch_cond = pitch_cond_hat = torch.argmax(pitch_cond_hat.squeeze(), dim=1).long().unsqueeze(0)
        dur_hat = self.dur_pred(x, pitch_cond, semb, alpha=alpha).squeeze(-1)
        pitch_hat = pitch_function(self.pitch_pred(x, pitch_cond, semb).transpose(1, 2))
        energy_hat = energy_function(self.energy_pred(x, semb).transpose(1, 2))
        return {'dur': dur_hat, 'pitch': pitch_hat, 'energy': energy_hat, 'pitch_cond': pitch_cond_hat}

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x = batch['x']
        mel = batch['mel']
        dur = batch['dur']
        semb = batch['speaker_emb'].contiguous()
        mel_lens = batch['mel_len']
        pitch = batch['pitch']
        pitch_cond = batch['pitch_cond']
        energy = batch['energy']
        self._begin_forward(x)

        # the four predictors are independent of the trunk in training (it consumes the batch's targets,
        # multi_forward_tacotron.py:183-213) and their 128-step recurrences are latency-bound: side HIP stream,
        # concurrently with the trunk, as in the single-speaker model (autograd replays each backward node on the
        # stream of its forward)
        fork = self._fork_predictors(x.device, lambda: self._predict(x, semb, pitch_cond))
        mel_cl, post_cl = self._trunk(x, semb, dur, pitch, energy, mel_lens.to(device=x.device, dtype=torch.long))
        Tout = mel.size(2)
        x_post = ops.TransposePadFn.apply(post_cl, Tout, self.padding_value)
        x_mel = ops.TransposePadFn.apply(mel_cl, Tout, self.padding_value)
        return {'mel': x_mel, 'mel_post': x_post, **self._join_predictors(fork)}

    def generate(self, x: torch.Tensor, speaker_emb: torch.Tensor, alpha=1.0,
                 pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x,
                 energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda x: x) -> Dict[str, torch.Tensor]:
        self.eval()
        with torch.no_grad():
            self._require_device(x)
            speaker_emb = speaker_emb.contiguous()
            # the four predictors beside embedding + prenet CBHG (side stream), joined where the trunk needs them
            pred, late_inputs = self._generate_fork(
                x, lambda: self._predict(x, speaker_emb, None, alpha, pitch_function, energy_function))
            mel_cl, post_cl = self._trunk(x, speaker_emb, None, None, None, None, late_inputs=late_inputs)
            T = mel_cl.shape[1]
            return {'mel': H.transpose_pad_fwd(mel_cl, T, 0.0), 'mel_post': H.transpose_pad_fwd(post_cl, T, 0.0),
                    **pred, 'pitch_cond': pred['pitch_cond'].unsqueeze(1)}

    # -- generate_batch: what base.AcousticModel's driver needs from this model -----------------------------------
    def generate_batch(self, x: torch.Tensor, x_len: torch.Tensor, speaker_emb: torch.Tensor, alpha=1.0,
                       pitch_function: Callable[[torch.Tensor], torch.Tensor] = lambda p: p,
                       energy_function: Callable[[torch.Tensor], torch.Tensor] = lambda e: e) -> Dict[str, torch.Tensor]:
        """base.AcousticModel.generate_batch with one speaker row per item (speaker_emb float32 [B,S] on the device); the
        result also holds `pitch_cond` int64 [B,Tx]"""
        return super().generate_batch(x, x_len, alpha, pitch_function, energy_function, speaker_emb=speaker_emb)

    def _ragged_prenet(self, x, xl, semb):
        return ForwardTacotron._ragged_prenet(self, x, xl)                    # the speaker row joins behind the prenet

    def _ragged_regulate(self, h, pred, semb):
        B, Tx = pred['dur'].shape
        # the padding rows get their item's speaker row too, but their durations are 0: they never reach the regulator
        h = ops.ConcatColsFn.apply(h, None, semb, B, Tx, True)                # [Tx,B,2P] -> [B,Tx,2P+S]
        h = self._cond_add(h, pred['pitch'], pred['energy'], False)
        return regulate_and_decode(self, h, pred['dur'], pred['mel_len'])     # packed LSTM; syncs to size Tm

    _ragged_finish = ForwardTacotron._ragged_finish
