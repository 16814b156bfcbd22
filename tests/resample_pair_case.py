"""Shared by tests/test_resample_pair.py (CPU) and tests/test_gpu_resample_pair.py: shapes for k_resample_strip's two-output form
through acf_hip_op_im_resample_pair, each chosen for a property.  The pipeline launches that form for few geometries
(tests/scale_forms_case.py: B needs at most half of A's columns); the op aims at what those leave open: exact axes under <true, false>,
both outputs slow, B's tails, up to eight row tiles, nStepsB < nSteps inside a column segment and each refusal with the outputs still right.

A case: id -> (ha, wa, hbA, wbA, hbB, wbB, d, props, word)
  props  what the shape is chosen for, confirmed on the CPU from tap counts restated from the reference's resampleCoef
         (tests/level_forms_case.py axis_taps): "yA" / "xA" / "yB" / "xB": (kind, taps) wanted, kind alone where the count is not the point
  word   what the op must report: pair (launched) or the refusal, SLOW, nty, nty_b, n_split, n_steps, n_steps_b.  n_steps = ceil(wbA / 4),
         n_steps_b = ceil(wbB / 2) and the refusals but no_tiling are restated on the CPU; nty, nty_b and n_split need the whole tiling
         and are stated here for the report to agree with.  n_split comes out of launchStrip's cost model over the device's CU count and LDS
         per CU: the figures are the MI355X's (256 CUs, 160 KB) and hold on no other device.
No source exceeds 640 x 128 floats per plane.  The reference: two acfo_resample calls, compared as bits at nrm 1.0 and 1.0832."""
import level_forms_case as lf

NRMS = (1.0, 1.0832)
RS_XO = 4


def launched(slow, nty, nty_b, n_split, n_steps, n_steps_b):
    return dict(pair=True, why=None, slow=slow, nty=nty, nty_b=nty_b, n_split=n_split, n_steps=n_steps, n_steps_b=n_steps_b)


def refused(why):
    return dict(pair=False, why=why, slow=False, nty=0, nty_b=0, n_split=0, n_steps=0, n_steps_b=0)


CASES = {
    # <true, false>
    "fast_neither_exact": (104, 80, 80, 62, 40, 31, 2, dict(yA="down", xA="down", yB="down", xB="down"), launched(False, 1, 1, 2, 16, 16)),
    "fast_b_exact4_a_exact_x": (96, 96, 70, 48, 24, 24, 2, dict(yA="down", xA="exact", yB="exact", xB="exact"), launched(False, 1, 1, 1, 12, 12)),
    "fast_b_exact3_y": (96, 96, 70, 48, 32, 24, 2, dict(yA="down", xA="exact", yB="exact", xB="exact"), launched(False, 1, 1, 1, 12, 12)),
    # <true, true>
    "slow_b_only": (128, 64, 60, 32, 28, 16, 2, dict(yA="down", yB="down", slowA=False, slowB=True), launched(True, 1, 1, 1, 8, 8)),
    "slow_both_anisotropic": (200, 64, 62, 48, 31, 24, 2, dict(yA="down", yB="down", slowA=True, slowB=True), launched(True, 1, 1, 1, 12, 12)),
    # B's tails: every residue of wbA mod 4 with wbB odd and even; odd heights
    "wa0_wb_odd": (64, 48, 44, 40, 21, 19, 2, {}, launched(False, 1, 1, 1, 10, 10)),
    "wa0_wb_even": (64, 48, 44, 40, 21, 20, 2, {}, launched(False, 1, 1, 1, 10, 10)),
    "wa1_wb_odd": (64, 48, 44, 41, 21, 19, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "wa1_wb_even": (64, 48, 44, 41, 21, 20, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "wa2_wb_odd": (64, 48, 44, 42, 21, 19, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "wa2_wb_even": (64, 48, 44, 42, 21, 20, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "wa3_wb_odd": (64, 48, 44, 43, 21, 19, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "wa3_wb_even": (64, 48, 44, 43, 21, 20, 2, {}, launched(False, 1, 1, 1, 11, 10)),
    "heights_odd": (64, 48, 45, 40, 21, 20, 2, {}, launched(False, 1, 1, 1, 10, 10)),
    # B's steps against A's: equal (wa0_wb_even), below, one above (refused)
    "b_steps_below": (64, 48, 44, 40, 21, 17, 2, {}, launched(False, 1, 1, 1, 10, 9)),
    "b_steps_above": (64, 48, 44, 40, 21, 21, 2, {}, refused("b_steps")),
    # row tiles: nty 1 above; 3 with ntyB = nty; 5 with ntyB 4; 8 with ntyB 5 and B slow
    "nty3_equal": (640, 32, 320, 20, 160, 10, 2, {}, launched(False, 3, 3, 1, 5, 5)),
    "nty5_b4": (640, 32, 600, 24, 215, 12, 2, {}, launched(False, 5, 4, 1, 6, 6)),
    "nty8_b5_slow": (640, 32, 330, 20, 100, 10, 2, dict(slowA=False, slowB=True), launched(True, 8, 5, 1, 5, 5)),
    # column segments: 20 steps in 2 segments of 10; B has 18, so the second segment runs 8 steps of B beside 10 of A.  d = 1, 2, 3
    "split2_d1": (128, 96, 100, 80, 50, 36, 1, {}, launched(False, 1, 1, 2, 20, 18)),
    "split2_d2": (128, 96, 100, 80, 50, 36, 2, {}, launched(False, 1, 1, 2, 20, 18)),
    "split2_d3": (128, 96, 100, 80, 50, 36, 3, {}, launched(False, 1, 1, 2, 20, 18)),
    "split5_nty2_d3": (128, 192, 100, 160, 50, 60, 3, {}, launched(False, 2, 2, 5, 40, 30)),
    # the smallest source, and the refusals
    "ha8": (8, 64, 5, 40, 3, 20, 2, {}, launched(False, 1, 1, 1, 10, 10)),
    "ha10_rows": (10, 64, 5, 40, 3, 20, 2, {}, refused("rows")),
    "x_equal_not_down": (128, 96, 100, 96, 50, 36, 3, dict(xA="up"), refused("not_down")),
    "b_x_taps": (64, 96, 44, 40, 21, 19, 2, dict(xB=("down", 6)), refused("x_taps")),
    "b_slow_taps": (400, 64, 44, 40, 41, 20, 2, {}, refused("slow_taps")),
    "no_tiling_b_taller_than_half": (120, 64, 25, 48, 23, 24, 2, dict(slowA=True, slowB=True), refused("no_tiling")),
}


def axes(ha, wa, hb, wb):
    return lf.axis_taps(ha, hb), lf.axis_taps(wa, wb)


def slow(ha, hb):
    kind, taps = lf.axis_taps(ha, hb)
    return kind == "down" and taps > 4


def cheap_reason(ha, wa, hbA, wbA, hbB, wbB):
    """stripPlan's refusal of the pair in its order, as far as tap counts tell (None: launched, or no_tiling)"""
    ax = [axes(ha, wa, hbA, wbA), axes(ha, wa, hbB, wbB)]
    if any(k == "up" for yx in ax for k, _ in yx):
        return "not_down"
    if ha % 4 or ha < 8:
        return "rows"
    if any(y[0] == "down" and y[1] > 8 for y, _ in ax):
        return "slow_taps"
    if any(x[0] == "down" and x[1] > 4 for _, x in ax):
        return "x_taps"
    if -(-wbB // (RS_XO // 2)) > -(-wbA // RS_XO):
        return "b_steps"
    return None
