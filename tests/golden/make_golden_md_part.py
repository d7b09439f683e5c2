"""Writes tests/golden/md_part.npz: what the reference's own d1_non_square_block_decision, d2_inter_depth_block_decision and the walk of
EncodePass give for the cases of tests/md_part_util.py (through tests/golden/ref_md_part_driver.c; needs the reference and
oracle/_ref/obj_all).  Per case and superblock: a digest of cost, part, split_flag, best_d1_blk, tested_cu_flag and mdc_split_flag over all
md-scan indices, the final md-scan indices in coding order, and the driver's count of the Av1SplitFlagRate arms.  The inputs are not stored:
md_part_util makes them from the case's name.

The generator fails unless, on the reference's results: our block table equals blk_geom_mds field by field for both superblock sizes; the
restatement equals the reference on every superblock; every Av1SplitFlagRate call took the hasRows && hasCols arm (or was below 8x8, where
no context is read either); and the cases hold what they are for (md_part_util.assert_coverage): every PartitionType a square size allows
wins somewhere at that size, split and not-split at every depth, a d1 tie (strict <) and a d2 tie (<=), an intra root with a stale non-zero
cost, MAX_MODE_COST shapes in an incomplete superblock."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import md_part_util as pu  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = pu.build_reference_driver(tmp)
        for sb_size in (64, 128):
            ref, ours = pu.reference_geometry(L, sb_size), pu.geometry(sb_size)
            assert len(ref) == len(ours) == (4421 if sb_size == 128 else 1101)
            assert int((ours["shape"] == 0).sum()) == (1365 if sb_size == 128 else 341)
            for i, field in enumerate(pu.REF_GEOM_FIELDS):
                assert np.array_equal(ref[:, i], ours[field].astype(np.int32)), (sb_size, field)
            out[f"geometry{sb_size}"] = np.array(pu.digest(ref))
        arms = np.zeros(4, np.int64)
        for name in pu.CASES:
            s, e = pu.scenario(name), pu.expected(name)
            digests, finals, counts = [], [], []
            for k in range(len(s.origins)):
                r, counters = pu.reference_walk(L, s, k)
                w = e["walks"][k]
                for key in ("cost", "part", "split", "best", "tested", "mdc", "final"):
                    assert r[key] == w[key], (name, k, key, [(i, a, b) for i, (a, b) in enumerate(zip(r[key], w[key])) if a != b][:5])
                assert counters[1] == counters[2] + counters[3], (name, k, counters)
                arms += counters
                digests.append(pu.state_digest(r)), finals.extend(r["final"]), counts.append(len(r["final"]))
            out[f"{name}__state"], out[f"{name}__final"], out[f"{name}__count"] = np.array(digests), np.array(finals, np.uint16), np.array(counts, np.uint32)
    # a 4x4 never gets a rate of its own (its leaf is not larger than 4x4), so no call is below 8x8: all of them took the inside arm
    assert arms[1] > 0 and arms[1] == arms[2] and arms[3] == 0, arms
    out["split_flag_rate_arms"] = arms[1:]
    stats = pu.assert_coverage(pu.CASES)
    assert pu.expected("p64-leafless-p-v0")["refused"] == 1
    path = os.path.join(ROOT, "tests", "golden", "md_part.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(pu.CASES)} cases, {os.path.getsize(path)} bytes; Av1SplitFlagRate calls {arms[1]} ({arms[2]} inside, {arms[3]} below 8x8); {stats}")


if __name__ == "__main__":
    main()
