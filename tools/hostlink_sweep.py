#!/usr/bin/env python3
"""Grid sweep and default-size run of the host-link probe on one GPU.

Sweeps the workgroup count of the three hostlink kernels (fill = GPU
stores to pinned host memory, verify = GPU loads from it, duplex = both
in one launch) at one buffer size, then runs hostlink() once at its
default size, and writes everything as one JSON file — the source of
profiles/hostlink_mi355x.json and of the default grids in
csrc/hostlink.hip (the smallest grid within 2 % of the best).

    python tools/hostlink_sweep.py --out profiles/hostlink_mi355x.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRIDS = (8, 16, 32, 64, 128, 256, 512, 1024)
SPEC_GBPS = 63.0  # PCIe Gen5 x16, discovery/types.py PCIE_GBPS_DEFAULT


def _time(fn, iters):
    import torch

    fn()  # warm-up: code object load, first touch
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()  # every entry point returns after its stream synchronise
        times.append(time.perf_counter() - t0)
    return times


def _row(blocks, moved, times):
    return {
        "blocks": blocks,
        "gbps": round(moved * len(times) / sum(times) / 1e9, 3),
        "best_gbps": round(moved / min(times) / 1e9, 3),
        "times_ms": [round(t * 1e3, 3) for t in times],
    }


def _smallest_within(rows, share=0.02):
    best = max(r["gbps"] for r in rows)
    return min(r["blocks"] for r in rows if r["gbps"] >= (1.0 - share) * best)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)

    import torch

    from kubegpu_amd.probe import hostlink as hl

    if not torch.cuda.is_available():
        print("hostlink_sweep: no GPU visible", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    n = args.bytes
    half = n // 2
    H = hl.alloc(n)
    lower, upper = H[:half], H[half:]
    out = {
        "device": torch.cuda.get_device_name(0),
        "bytes": n,
        "iters": args.iters,
        "timing": "perf_counter around one call that ends in a stream "
                  "synchronise; gbps = bytes * iters / sum(times), one warm-up first",
        "built_defaults": dict(zip(("read_blocks", "write_blocks"), hl.default_blocks())),
        "fill": [], "verify": [], "duplex": [], "duplex_at_defaults": None,
    }
    for b in GRIDS:
        out["fill"].append(_row(b, n, _time(
            lambda: hl.fill_pattern(H, "addr", 1, blocks=b), args.iters)))
    for b in GRIDS:  # H holds addr from the last fill
        res = []
        out["verify"].append(_row(b, n, _time(
            lambda: res.append(hl.verify_pattern(H, "addr", 1, blocks=b)), args.iters)))
        assert all(r.ok for r in res), "verify sweep saw mismatches"
    hl.fill_pattern(lower, "checker", 1)
    for b in GRIDS:  # b workgroups per direction; half the buffer each way
        res = []
        out["duplex"].append(_row(b, n, _time(
            lambda: res.append(hl.duplex(lower, "checker", upper, "walk1", 1,
                                         read_blocks=b, write_blocks=b)), args.iters)))
        assert all(r.ok for r in res), "duplex sweep saw mismatches"
    # the duplex kernel as the probe launches it: each side's own default
    res = []
    out["duplex_at_defaults"] = _row(0, n, _time(
        lambda: res.append(hl.duplex(lower, "checker", upper, "walk1", 1)), args.iters))
    assert all(r.ok for r in res), "duplex at the default grids saw mismatches"
    out["smallest_within_2pct"] = {k: _smallest_within(out[k])
                                   for k in ("fill", "verify", "duplex")}
    del lower, upper, H

    t0 = time.perf_counter()
    result = hl.hostlink()  # default size, allocation included in the wall time
    wall = time.perf_counter() - t0
    d = result.to_dict()
    out["default_run"] = {
        "wall_s_including_allocation": round(wall, 4),
        "result": d,
        "share_of_63_gbps_spec": {
            k: round(d[k] / SPEC_GBPS, 3)
            for k in ("kernel_h2d_gbps", "kernel_d2h_gbps", "copy_h2d_gbps",
                      "copy_d2h_gbps")
        },
        "duplex_share_of_2x63_gbps": round(d["duplex_gbps"] / (2 * SPEC_GBPS), 3),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"smallest_within_2pct": out["smallest_within_2pct"],
                      "default_run": {k: v for k, v in out["default_run"].items()
                                      if k != "result"},
                      "ok": d["ok"]}))
    return 0 if d["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
