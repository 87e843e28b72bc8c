#!/usr/bin/env python3
"""Record what the real library (oracle/_ref) answers on the 64 edge-case pairs for every configuration of tests/oracle_configs.py
-> tests/golden/oracle_grid.json (sha256 of statuses, scores and op strings per configuration; recorded results only).

    python tools/make_oracle_grid_golden.py

A row is recorded only if the oracle agrees with the library on it.  The rows the library has no defined answer for never reach it."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import common  # noqa: E402
import oracle_configs as oc  # noqa: E402
from oracle import loader  # noqa: E402


def main():
    path = os.path.join(ROOT, "tests", "golden", "oracle_grid.json")
    out = {}
    for name, e in sorted(oc.registry().items()):
        if e["undefined"]:
            continue
        cfg, mini = oc.mini_config(e)
        r = loader.run(loader.reference(), cfg, mini)
        o = loader.run(loader.oracle(), cfg, mini)
        common.assert_same(r, o["score"], o["status"], o["cigars"], mini, f"oracle vs reference {name}")
        out[name] = oc.digest(r)
    with open(path, "w") as f:
        json.dump({"corpus": "corpus_common.special_mini(validate_oracle.corpus_special(seed=99))", "digests": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} configurations recorded -> {path}")


if __name__ == "__main__":
    main()
