"""Superseded.  The statistics of the counter-based dropout mask (keep rate, lags, residue classes of the index, the
independence of consecutive stream seeds, index avalanche, the seed limits) are asserted by tests/test_dropout_cpu.py on
the numpy restatement tests/dropout_cpu.py, which tests/test_gpu_dropout.py holds bit for bit to the kernels:

    python -m pytest -s tests/test_dropout_cpu.py        # prints every figure, needs no GPU
"""
