"""The tile-order arithmetic (csrc/tile_order_host.h: the centre-out sort, the
cost orders of tile orders 3 / 4 / 5, the effective costs, the split count
and the held fine region) on the CPU, under the address and
undefined-behaviour sanitizers.  tests/tile_order_main.cpp checks the
invariants of every output and that its hash equals the one recorded in
tests/golden/tile_order.json -- from the functions as they stood inside
rt_api.cpp before they moved, so the arithmetic is the same bit for bit."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_order_invariants_and_recorded_hashes(tmp_path):
    with open(os.path.join(HERE, "golden", "tile_order.json")) as fp:
        cases = json.load(fp)["cases"]
    exe = str(tmp_path / "tile_order_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "tile_order_main.cpp")], check=True)
    argv = [exe]
    for c in cases:
        argv += ["case"] + [f"{k}={v}" for k, v in c.items()]
    r = subprocess.run(argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases ok" in r.stdout
