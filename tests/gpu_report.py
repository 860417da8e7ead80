"""The parity report of the GPU tests: one JSON line per case, appended to parity_report.jsonl in the GPU model tests' output
directory (measured errors beside their gates; never asserted on)."""
import json
import os

from tests.test_gpu_model import OUT


def note(name, payload):
    try:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "parity_report.jsonl"), "a") as f:
            f.write(json.dumps(dict(case=name, **payload)) + "\n")
    except OSError:
        pass
