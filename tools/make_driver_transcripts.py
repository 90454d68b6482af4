#!/usr/bin/env python3
"""CPU: records ``tests/golden/optimizer_driver_transcripts.json`` -- what every ``TemplateOptimizer._run_batch*`` strategy asks of its
contexts (one transcript per context), what it returns and the statistics it leaves, against the recording stand-in of
``tests/fake_ctx.py`` (the cases are ``fake_ctx.CASES``; neither the library nor a GPU is needed).  The file is the project's own
recorded behaviour at the commit it was made at: ``tests/test_optimizer_driver_host.py`` holds later trees to it.

    python tools/make_driver_transcripts.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fake_ctx  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "optimizer_driver_transcripts.json")
    cases = {name: run()[0] for name, run in fake_ctx.CASES.items()}
    with open(out, "w") as f:
        json.dump(cases, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
