"""Records tests/golden/trajectory_front.json: the message of every malformed call of tests/test_trajectory_front.py, as the checked-out
tree gives them.  It was run on the commit before gym_amd/_trajectory_args.py and gym_amd/csrc/mxv_trajectory.hpp existed; to run it
again is to accept the present messages as the reference.

    python tests/golden/make_trajectory_front.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
import test_trajectory_front as front  # noqa: E402

golden = {"messages": {key: front.message_of(key) for key in sorted(front.CASES)}}
with open(front.GOLDEN, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(golden['messages'])} messages -> {front.GOLDEN}")
