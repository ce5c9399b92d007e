"""Summarise rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `python bench.py` into profiles/<name>.json.

Usage (on the GPU box, two separate passes as MI355X_MICROARCH.md prescribes — FETCH_SIZE and WRITE_SIZE do not fit one pass):
  rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d pmc_fetch -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline
  rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d pmc_write -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline
  python tools/pmc_traffic.py pmc_fetch pmc_write gemm_nt_ gemm_traffic.json

Corrections (guide, HBM section): both counters are in KB; on gfx950 FETCH_SIZE counts 128-B requests at 64 B, so it is doubled;
WRITE_SIZE is exact.  Infinity-Cache hits are included in FETCH_SIZE (fabric-side requests), so `traffic` is an upper bound on HBM bytes.
"""
import csv
import glob
import json
import sys
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "rga3-release_amd"))
from rga3.utils.fingerprint import tree_fingerprint


def per_kernel(d, counter, needle):
    tot, n = 0.0, 0
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == counter and needle in row["Kernel_Name"]:
                    tot += float(row["Counter_Value"])
                    n += 1
    return tot, n


def main():
    dfetch, dwrite, needle, out = sys.argv[1:5]
    f, nf = per_kernel(dfetch, "FETCH_SIZE", needle)
    w, nw = per_kernel(dwrite, "WRITE_SIZE", needle)
    res = {"kernel": needle, "launches_fetch_pass": nf, "launches_write_pass": nw,
           "fetch_bytes_per_launch": 2.0 * 1024.0 * f / max(nf, 1), "write_bytes_per_launch": 1024.0 * w / max(nw, 1),
           "corrections": "KB->B; FETCH_SIZE x2 on gfx950 (128-B requests tallied at 64 B); WRITE_SIZE exact; Infinity-Cache hits included"}
    res["traffic_bytes_per_launch"] = res["fetch_bytes_per_launch"] + res["write_bytes_per_launch"]
    res["tree"] = tree_fingerprint()     # bench.py quotes this file only while the running tree has the same fingerprint
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
