"""The expected result of a fused call with the box fit (rule C24) on, composed on the CPU: the records of tests/prism_reference.py
(the oracle's front end, rule C20 and rule C16 when they are on, the oracle's clustering and ICP) or, for a depth-fed call, of
tests/fused_reference.py, and for every cluster perception_amd/box_fit.py on (the frame's plane, the cluster's points as
extracted).  The rule changes no record of the call, so everything the composed reference returns stays and every frame gains
"box_fits".  CPU only."""
import numpy as np

import fused_reference as FR
import prism_reference as PR
from perception_amd import box_fit as BF, capi


def fits_of(e, band):
    have = e["status"] == capi.CD_OK and e["counts"][2] > 0
    return [BF.box_fit(e["plane"], c.points, band, have_plane=have) for c in e["clusters"]]


def expected(frames, prm, templates_by_slot, band=BF.BAND_DEFAULT, prism=None, filter=None, keys=None):
    out = PR.expected(frames, prm, templates_by_slot, prism=prism, filter=filter, keys=keys)
    for e in out:
        e["box_fits"] = fits_of(e, band)
    return out


def expected_depth(depth, color, cam, prm, templates_by_slot, band=BF.BAND_DEFAULT):
    out = FR.expected((depth, color), prm, templates_by_slot, FR.options(cam=cam))
    for e in out:
        e["box_fits"] = fits_of(e, band)
    return out


def expected_selection(frame, prm, templates_by_slot, slot_dims, tolerance, band=BF.BAND_DEFAULT):
    """One frame of a template_slot = -1 call with the selection on, composed from one oracle run per slot (as tests/test_gpu_scale.py
    composes config 5): a list, per cluster, of dict(box = the module's record with match_slot / match_cost filled, slot = the slot
    the call must report, result = that slot's oracle cluster result, all_pairs_slot = the slot the call without the selection
    keeps - the lowest fitness, a tie to the lowest slot).  A cluster whose record is CD_OK and matches a loaded slot takes that
    slot alone; every other the all-pairs one."""
    from oracle import oracle_py as O
    slots = sorted(templates_by_slot)
    per = {}
    for s in slots:
        q = FR.copy_params(prm)
        q.template_slot = s
        per[s] = O.process_frame(frame, q, templates_by_slot[s], want_clouds=True, all_clusters=64)
    o = per[slots[0]]
    r = o["result"]
    plane = np.array(list(r.plane), np.float32)
    mask = sum(1 << s for s in slots)
    out = []
    for k in range(r.n_clusters):
        pts = np.ascontiguousarray(o["objects"][o["labels"] == k])
        box = BF.box_fit(plane, pts, band, have_plane=r.n_plane > 0)
        if box["status"] == capi.CD_OK:
            box["match_slot"], box["match_cost"] = BF.match(box["dims"], slot_dims, mask, tolerance)
        best = min(slots, key=lambda s: (per[s]["clusters"][k].fitness, s))
        slot = box["match_slot"] if box["match_slot"] >= 0 else best
        out.append(dict(box=box, slot=slot, result=per[slot]["clusters"][k], all_pairs_slot=best, all_pairs_result=per[best]["clusters"][k], points=pts))
    return out
