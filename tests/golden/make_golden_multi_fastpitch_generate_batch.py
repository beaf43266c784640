"""Fixture of MultiFastPitch.generate_batch: tests/golden/multi_fastpitch_generate_batch.npz.

Needs the reference checkout (FT_REFERENCE, as make_golden.py).  The tiny MultiFastPitch config of
make_golden_multi_fastpitch.py; content, batch and seed-search conditions are those of
make_golden_multi_generate_batch.py, whose functions build it.  The pitch_cond logits are stored as generate() forms
them, divided by alpha (multi_fast_pitch.py:255).  The `pe` buffers are stored truncated to PE_ROWS rows
(helpers.fp_state rebuilds them).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_fastpitch import PE_ROWS, put_sd  # noqa: E402  (puts the reference checkout on sys.path)
from make_golden_multi_fastpitch import TINY_MFP  # noqa: E402
from make_golden_multi_generate_batch import ALPHA, search  # noqa: E402
from models.multi_fast_pitch import MultiFastPitch  # noqa: E402

DUR_SCALE, DUR_BIAS = 3.0, 2.5       # as make_golden_fastpitch_generate_batch.py


def main():
    import numpy as np

    def put_state(out, sd):
        out['pe_rows'] = np.int64(PE_ROWS)
        put_sd(out, 'sd/', sd)

    search('multi_fastpitch_generate_batch.npz', MultiFastPitch, TINY_MFP, DUR_SCALE, DUR_BIAS,
           lambda m, x, s: m.pitch_cond_pred(x, speaker_emb=s, alpha=ALPHA), put_state)


if __name__ == '__main__':
    main()
