"""tests/golden/level_decoder_refusals.tsv: what every row of tests/level_refusal_cases.py raises (Python entries: exception type and message) or returns (the four C
entry points: the status code), on a machine WITHOUT a device and with the library built.

    python tools/gen_level_decoder_refusals.py > tests/golden/level_decoder_refusals.tsv

The committed table was written once, before the host paths of the level-weighted decoders were merged (one prelude per operation in codec.py, one flow in detect.py, one
check function in csrc/gswm_codec_soft.inc); tests/test_level_decoder_refusals.py replays the rows against the current code and does not run this tool.  After a deliberate
change of a refusal, run it again: the diff of the table is the change."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import level_refusal_cases as L  # noqa: E402

if torch.cuda.is_available():
    sys.exit("run this on a machine without a device: the made-up pointers of the C rows must never meet one")
print("entry\ttag\twhere\toutcome\tmessage")
for entry, tag, where, thunk in L.CASES:
    kind, message = L.outcome(thunk, where)
    assert "\t" not in message
    print(f"{entry}\t{tag}\t{where}\t{kind}\t{message}")
for symbol, tag, made_up, args in L.C_CASES:
    print(f"{symbol}\t{tag}\t{'made_up' if made_up else 'null'}\tstatus\t{L.c_outcome(symbol, args)}")
