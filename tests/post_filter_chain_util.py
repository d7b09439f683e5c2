"""The post-reconstruction filter chain as one run of the restatements, for tests/test_post_filter_chain_vs_ref.py and
tests/test_post_filter_chain_gpu.py.  TEST INFRASTRUCTURE: numpy only, no reference code.

  deblocking level pick -> deblocking -> CDEF search and pick -> CDEF -> Wiener search, self-guided search -> restoration -> film grain

Every stage is the frame-level restatement of its own util (dlf_util, cdef_util, lr_util, lr_sgr_util, film_grain_util), each pinned to
the reference alone; here each is fed what the stage before it left.  The restoration unit types stand in for the host's
rest_finish_search, which is not on the device: unit_type[u] = u % 3, so every plane of a 2 x 2 unit picture holds RESTORE_NONE,
RESTORE_WIENER and RESTORE_SGRPROJ units.  Taps and self-guided parameters are always the searches' own results.

The three pictures are 200 x 200: 4 x 4 CDEF filter blocks with an 8-sample last column and row, 2 x 2 restoration units per plane (unit
sizes 128 / 64 / 64), stripes with substituted rows above, below and on both sides, nothing a multiple of 64.  They are regenerated from
their seeds; tests/golden/post_filter_chain.npz holds digests of the inputs and what the reference's own chain made of them."""
import hashlib
import os

import numpy as np

import cdef_util as cu
import dlf_util as du
import film_grain_util as fu
import lr_sgr_util as su
import lr_util as lu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "post_filter_chain.npz")
W = H = 200
# picture B's base_qindex: damping 3 + (160 >> 6) = 5
PICTURES = {"A": {"seed": 3, "bd": 8, "last_levels": (20, 20, 20, 20), "base_qindex": 100, "grain_set": 4},
            "B": {"seed": 4, "bd": 10, "last_levels": (20, 20, 20, 20), "base_qindex": 160, "grain_set": 5},
            "C": {"seed": 0, "bd": 8, "last_levels": (0, 0, 0, 0), "base_qindex": 100, "grain_set": 4}}
PARAM_KEYS = ("seed", "bd", "base_qindex", "grain_set")
PLANE_STAGES = ("dbk", "cdef", "restored", "grain")
# the small results in chain order: (name, dtype)
SMALL = (("levels", np.int32), ("masks", np.uint64), ("mse", np.uint64), ("counted", np.uint8), ("cdef_result", np.int32), ("fb_strength", np.int8),
         ("wiener_sse", np.int64), ("taps", np.int16), ("n_trials", np.int32), ("sgrproj", np.int32), ("sgr_sse", np.int64), ("unit_type", np.uint8))


def make_picture(name):
    """(mi, recon planes, source planes) of picture `name`, from its seed"""
    P = PICTURES[name]
    rng = np.random.default_rng(P["seed"])
    mi = du.random_mi_grid(rng, W, H)
    recon, source = du.random_picture(rng, W, H, P["bd"], mi)
    return mi, recon, source


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def input_digests(mi, recon, source):
    """sha256 of the reconstruction, the source and the mode-info grid: the proof that a box regenerated the fixture's input"""
    return {"recon": sha256(*recon), "source": sha256(*source), "mi": sha256(mi)}


def skip_map(mi, w=W, h=H):
    """one byte per 4x4 luma cell of the picture: the skip flag of the mode-info grid, cut to the picture"""
    return np.ascontiguousarray((mi["flags"] & 1)[:h // 4, :w // 4].astype(np.uint8))


def unit_types(n_units):
    return (np.arange(n_units) % 3).astype(np.uint8)


def run_chain(recon, source, mi, bd, last_levels, base_qindex, grain_set, w=W, h=H):
    """every intermediate of the restated chain: the SMALL arrays, the PLANE_STAGES plane triples, and `rejected` [units]"""
    out = {}
    levels, masks, _ = du.pick_filter_level(recon, source, mi, last_levels, 0, 0, bd)
    out["levels"], out["masks"] = np.array(levels, np.int32), np.array(masks, np.uint64)
    dbk = [p.copy() for p in recon]
    du.loop_filter_frame(dbk, mi, levels, 0, 0, 3, bd)
    out["dbk"] = dbk

    skip = skip_map(mi, w, h)
    mse, counted, _, _ = cu.search(dbk, source, skip, w, h, bd, base_qindex)
    res, fbs = cu.pick(mse, counted, base_qindex, bd)
    out["mse"], out["counted"], out["cdef_result"], out["fb_strength"] = mse, counted, res.reshape(1).view(np.int32).copy(), fbs
    cdef = cu.frame(dbk, skip, w, h, bd, res, fbs)
    out["cdef"] = cdef

    planes, base = lu.picture_units(w, h)
    n = base[3]
    sse, taps, ntr = np.zeros((n, 2), np.int64), np.zeros((n, 16), np.int16), np.zeros(n, np.int32)
    sgr, sgr_sse, rejected = np.zeros((n, 4), np.int32), np.zeros(n, np.int64), np.zeros(n, bool)
    for p in range(3):
        win, ss = (7, 5)[p > 0], int(p > 0)
        for i, lim in enumerate(planes[p][0]):
            u = base[p] + i
            M, Hm, _ = lu.compute_stats(cdef[p], source[p], lim, win, bd)
            vf, hf, rej = lu.solve(M, Hm, win)
            sse[u, 0], sse[u, 1], rejected[u] = lu.unit_sse(cdef[p], source[p], lim), lu.INT64_MAX, rej
            if not rej:
                err, vf, hf, trace = lu.walk(lambda a, b: lu.trial_sse(cdef[p], dbk[p], source[p], lim, a, b, bd, ss), vf, hf, win)
                sse[u, 1], taps[u], ntr[u] = err, vf + hf, len(trace)
            _, _, best = su.search_unit(cdef[p], source[p], lim, bd, ss, keep_trace=False)
            sgr[u, :3] = best
            sgr_sse[u] = su.trial_sse(cdef[p], dbk[p], source[p], lim, best[0], best[1:], bd, ss)     # sse[RESTORE_SGRPROJ]
    out["wiener_sse"], out["taps"], out["n_trials"], out["sgrproj"], out["sgr_sse"], out["rejected"] = sse, taps, ntr, sgr, sgr_sse, rejected
    out["unit_type"] = unit_types(n)
    out["restored"] = su.filter_frame(cdef, dbk, w, h, bd, (1, 1, 1), out["unit_type"], taps, sgr)
    out["grain"] = fu.add_film_grain(fu.PARAM_SETS[grain_set], bd, *out["restored"], t=fu.tables_of(grain_set, bd))
    return out


def chain_of(name):
    """(mi, recon, source, the restated chain) of picture `name`"""
    P = PICTURES[name]
    mi, recon, source = make_picture(name)
    return mi, recon, source, run_chain(recon, source, mi, P["bd"], P["last_levels"], P["base_qindex"], P["grain_set"])


def conditions(name, recon, chain):
    """what the issue asks of the pictures, as {condition: holds}; evaluated on the restatement's chain, never on the device's"""
    levels = [int(v) for v in chain["levels"]]
    if name == "C":
        return {"luma levels are 0": levels[0] == 0 and levels[1] == 0, "a chroma level is not 0": levels[2] != 0 or levels[3] != 0,
                "deblocking leaves every plane": all(np.array_equal(a, b) for a, b in zip(chain["dbk"], recon))}
    res = chain["cdef_result"].view(cu.RESULT_DTYPE)[0]
    planes, base = lu.picture_units(W, H)
    stages = [recon] + [chain[k] for k in PLANE_STAGES]
    ok = {"all four levels are not 0": all(levels), "cdef_bits > 0": int(res["cdef_bits"]) > 0,
          "a filter block is left out of the CDEF search": bool((chain["fb_strength"] == -1).any()),
          "every Wiener walk makes more than one trial": bool((chain["n_trials"] > 1).all()),
          "every plane has units of all three types": all(set(chain["unit_type"][base[p]:base[p + 1]].tolist()) == {0, 1, 2} for p in range(3))}
    for k, (a, b) in zip(PLANE_STAGES, zip(stages, stages[1:])):
        ok[f"{k} changes samples in all three planes"] = all(not np.array_equal(x, y) for x, y in zip(a, b))
    return ok


# ---------------------------------------------------------------- the fixture
def plane_digest(planes):
    return np.array([fu.digest(planes)], np.uint64)


_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        _FIXTURE.update(np.load(FIXTURE))
    return _FIXTURE


def expected(name, recon=None):
    """what the fixture holds of picture `name`: the SMALL arrays, sha256 of the inputs, `digest_<stage>` of every plane stage and, for a
    picture kept whole (`recon` needed: the planes are stored as differences against the stage before), the stage's planes"""
    z = fixture()
    out = {k: z[f"{name}_{k}"] for k, _ in SMALL}
    for k in PARAM_KEYS:
        out[k] = int(z[f"{name}_{k}"])
    out["last_levels"] = tuple(int(v) for v in z[f"{name}_last_levels"])
    for k in ("recon", "source", "mi"):
        out["sha256_" + k] = z[f"{name}_sha256_{k}"]
    prev = recon
    for k in PLANE_STAGES:
        out["digest_" + k] = z[f"{name}_digest_{k}"]
        if f"{name}_{k}_d0" in z and prev is not None:
            prev = out[k] = [(prev[p].astype(np.int32) + z[f"{name}_{k}_d{p}"]).astype(prev[p].dtype) for p in range(3)]
        else:
            prev = None
    return out


def first_difference(got, want, only=None):
    """the first stage, in chain order, at which `got` (arrays and plane triples by the names of SMALL and PLANE_STAGES) is not `want`
    (expected()), or among the names `only`: a string naming the stage and the plane or array, or None"""
    order = ("levels", "masks", "dbk", "mse", "counted", "cdef_result", "fb_strength", "cdef", "wiener_sse", "taps", "n_trials", "sgrproj", "sgr_sse",
             "unit_type", "restored", "grain")
    for k in order:
        if only is not None and k not in only:
            continue
        if k in PLANE_STAGES:
            if k in want:
                for p in range(3):
                    if not np.array_equal(got[k][p], want[k][p]):
                        at = np.argwhere(got[k][p] != want[k][p])
                        return f"{k}, plane {p}: {len(at)} samples differ, the first at (row, column) {at[0].tolist()}"
            elif plane_digest(got[k])[0] != want["digest_" + k][0]:
                return f"{k}: the digest of the three planes differs"
        else:
            g, w_ = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
            if g.shape != w_.shape or not np.array_equal(g.astype(w_.dtype), w_):
                at = np.flatnonzero(g.astype(w_.dtype) != w_)[:6] if g.shape == w_.shape else "shape"
                return f"{k}: differs at {at if isinstance(at, str) else at.tolist()}"
    return None
