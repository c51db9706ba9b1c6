#!/usr/bin/env python3
"""CPU trial behind the serial scan of hgs_strand_arclen (csrc/hgs_export.hip): how far a tree-shaped inclusive scan of the segment
lengths (64 lanes, Hillis-Steele, the carry added from chunk to chunk) lands from the definition's cum_{i+1} = cum_i + len_i, in
float64 units in the last place, over random strands with segment lengths of 0.1 to 6 mm (log-uniform).  numpy only; one JSON line."""
import json

import numpy as np


def tree_scan(v):
    v, d = v.copy(), 1
    while d < len(v):
        v = v + np.concatenate([np.zeros(d), v[:-d]])       # (lanes below d add +0: exact)
        d *= 2
    return v


def main():
    rng = np.random.default_rng(0)
    out = {}
    for n in (12, 80, 130):
        end, worst = [], []
        for _ in range(2000):
            seglen = 1e-4 * 60.0 ** rng.uniform(size=n)
            seq = np.cumsum(seglen)
            parts, carry = [], 0.0
            for b in range(0, n, 64):
                c = tree_scan(seglen[b:b + 64]) + carry
                parts.append(c)
                carry = c[-1]
            d = np.abs(np.concatenate(parts) - seq) / np.spacing(seq)
            end.append(d[-1])
            worst.append(d.max())
        end = np.asarray(end)
        out[str(n)] = {"L_rms_units": round(float(np.sqrt((end ** 2).mean())), 2), "L_max_units": float(end.max()),
                       "share_of_strands_beyond_4_units": round(float((end > 4).mean()), 4), "cum_max_units": float(max(worst))}
    print(json.dumps({"strands_per_size": 2000, "segments": out}))


if __name__ == "__main__":
    main()
