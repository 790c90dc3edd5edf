"""tests/golden/align_soft_l_refusals.tsv: what every row of tests/align_soft_l_refusal_cases.py raises (Python entries: exception type and message) or returns (the
two C entry points: the status code), on a machine WITHOUT a device and with the library built.

    python tools/gen_align_soft_l_refusals.py > tests/golden/align_soft_l_refusals.tsv

tests/test_align_soft_l_host.py replays the rows against the current code and does not run this tool.  After a deliberate change of a refusal, run it again: the diff
of the table is the change."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import align_soft_l_refusal_cases as L  # noqa: E402

if torch.cuda.is_available():
    sys.exit("run this on a machine without a device: the made-up pointers of the C rows must never meet one")
print("entry\ttag\twhere\toutcome\tmessage")
for entry, tag, where, thunk in L.CASES:
    kind, message = L.outcome(thunk, where)
    assert "\t" not in message
    print(f"{entry}\t{tag}\t{where}\t{kind}\t{message}")
for symbol, tag, made_up, args in L.C_CASES:
    print(f"{symbol}\t{tag}\t{'made_up' if made_up else 'null'}\tstatus\t{L.c_outcome(symbol, args)}")
