#!/usr/bin/env python3
"""One sha256 per case of the two split-K weight-streaming decode kernels (kernels/decode_stream.h), for comparing two builds of the
library on one MI355X: both kernels are deterministic and a refactor that keeps the order of every sum keeps every digest.

  linear  decodeLinear over the shapes, row counts and decorations of tests/test_generate_gpu.py::test_decode_linear_matches_f64, W as
          [K, N] and as [N, K]
  step    recurrentDecodeStep over the cases of tests/test_text_gpu.py::test_step_kernel_vs_module_and_restatement (the inputs are its
          _step_inputs): h, c and the relu copy

Usage: LAMP_LIB_PATH=<library> python scripts/decode_digest.py > digests.txt, once per build, then diff.  Needs an MI355X.  The digests
belong to one compiler and one device: they are compared, never committed."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd._capi import lib  # noqa: E402
lib.load()
import torch  # noqa: E402
import lamp_amd.languagemodel as L  # noqa: E402
from lamp_amd import text as TX  # noqa: E402
from tests.test_generate_gpu import DECORATIONS, _linear_case  # noqa: E402
from tests.test_text_gpu import KIND, STEP_SHAPES, _step_inputs  # noqa: E402
from tests.util import DTYPES, to_sten, to_torch  # noqa: E402


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    for dt in DTYPES:
        for K, N in [(12, 36), (13, 19), (48, 12), (3072, 768)]:
            for R in (1, 3, 16):
                for transposed in (False, True):
                    for what in DECORATIONS:
                        x, w, _, kw = _linear_case(dt, R, K, N, transposed, what)
                        out = to_torch(L.decodeLinear(to_sten(x), to_sten(w), transposed=transposed, **kw))
                        print(f"linear {dt} K={K} N={N} R={R} transposed={int(transposed)} {what} {digest(out)}", flush=True)
    for dt in (torch.float32, torch.float64):
        ts = lambda t: to_sten(t.to(dt))
        for kind in ("rnn", "gru", "lstm"):
            for n, (R, E, H) in enumerate(STEP_SHAPES):
                w, table, tok, state = _step_inputs(kind, dt, R, E, H, bool(n % 2))
                packed = TX.recurrentDecodePack(KIND[kind], [ts(t) for t in w])
                column = to_sten(torch.stack([tok, tok + 100], 1)).select(1, 0)             # tokens as a strided column, as the test passes them
                h, c, rl = TX.recurrentDecodeStep(KIND[kind], ts(table), column, packed, relu=True, hPrev=ts(state[0]),
                                                  cPrev=ts(state[1]) if kind == "lstm" else None)
                outs = [to_torch(h), to_torch(rl)] + ([to_torch(c)] if kind == "lstm" else [])
                print(f"step {dt} {kind} R={R} E={E} H={H} {digest(*outs)}", flush=True)


if __name__ == "__main__":
    main()
