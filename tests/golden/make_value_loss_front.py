"""Records tests/golden/value_loss_front.json: the message of every malformed call of tests/test_value_loss_front.py and the values of
workspace_bytes and launches, as the checked-out tree gives them.  It was run on the commit before gym_amd/_value_loss.py existed; to
run it again is to accept the present messages as the reference.

    python tests/golden/make_value_loss_front.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
import test_value_loss_front as front  # noqa: E402

golden = {"messages": {key: front.message_of(key) for key in sorted(front.CASES)}, "library": front.library_values()}
with open(front.GOLDEN, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(golden['messages'])} messages -> {front.GOLDEN}")
