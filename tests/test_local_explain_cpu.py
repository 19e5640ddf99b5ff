"""Local explanations, the parts that need no GPU: the argument checks of pipnet_local_explain_f32
(status before any HIP call) and the restatement of the reference loop (tests/local_explain_ref.py)
against a case worked by hand from util/visualize_prediction.py:63-88."""
import ctypes

import numpy as np
import torch

from count_pipnet_amd import _lib, build
from local_explain_ref import pack, reference_lists

PTR = ctypes.c_void_p(64)     # never dereferenced: every call below returns before a HIP call
POINTERS = ("pooled", "loc", "out", "w", "cls", "cls_logit", "n", "e_proto", "e_sim", "e_w", "e_simw", "e_loc")


def _lib_loaded():
    build.build()
    return _lib.load()


def _call(lib, b=1, p=8, k=5, c=3, m=4, ldw=None, min_abs=0.01, **null):
    ptr = {name: PTR for name in POINTERS}
    ptr.update(null)
    return lib.pipnet_local_explain_f32(ptr["pooled"], ptr["loc"], ptr["out"], ptr["w"], p if ldw is None else ldw,
                                        b, p, k, c, m, min_abs, ptr["cls"], ptr["cls_logit"], ptr["n"],
                                        ptr["e_proto"], ptr["e_sim"], ptr["e_w"], ptr["e_simw"], ptr["e_loc"], None)


def test_local_explain_rejects_bad_arguments_without_gpu():
    lib = _lib_loaded()
    for name in POINTERS:
        assert _call(lib, **{name: None}) == 1, name
        assert _call(lib, b=0, **{name: None}) == 1, name
    for bad in (0, -1):
        assert _call(lib, p=bad, ldw=8) == 1 and _call(lib, k=bad) == 1 and _call(lib, m=bad) == 1
    assert _call(lib, c=0) == 1 and _call(lib, c=-2) == 1
    assert _call(lib, k=5, c=6) == 1                               # C > K
    assert _call(lib, p=2049) == 1 and _call(lib, k=2049) == 1 and _call(lib, k=2049, c=2049) == 1
    assert _call(lib, p=8, ldw=7) == 1                             # ldw < P
    assert _call(lib, min_abs=-1e-9) == 1 and _call(lib, min_abs=float("nan")) == 1
    assert _call(lib, b=-1) == 1
    # the limits themselves are accepted (an empty batch launches nothing)
    assert _call(lib, b=0, p=2048, k=2048, c=2048, m=1) == 0
    assert _call(lib, b=0, p=8, ldw=8, min_abs=0.0) == 0


def test_local_explain_empty_batch_is_ok():
    lib = _lib_loaded()
    assert _call(lib, b=0) == 0 and _call(lib, b=0, p=1, k=1, c=1, m=1) == 0 and _call(lib, b=0, ldw=100) == 0


# ---- the restatement against a case worked by hand -------------------------------------------
# 2 images, 5 prototypes, 3 classes, 3 x 3 maps.  Products below are those of the float32 values
# (0.02f = 0.0199999995529651..., so 0.5f * 0.02f = 0.00999999977... is just NOT above 0.01).
F = np.float32
WEIGHT = [[0.02, 1.0, 0.01, 0.06, 0.0],
          [0.5, 0.0, 0.5, 0.04, 0.1],
          [0.0, 0.0, 0.0, -0.5, 0.5]]
POOLED = [[0.5, 0.0, 0.5, 0.2, 0.9],        # prototypes 0 and 2 tie: 0 comes first
          [0.0, 1.0, 0.0, 0.3, 0.0]]
OUT = [[1.0, 3.0, 2.0],                      # classes by logit: 1, 2, 0
       [2.0, 2.0, 1.0]]                      # classes 0 and 1 tie: 0 comes first
# where each prototype's map holds its maximum; prototype 3 of image 0 holds it twice, at (0, 2) and
# (2, 1): max over rows first, then the first column that has it -> (2, 1), not the row-major (0, 2)
PEAKS = [{0: [(1, 1)], 2: [(0, 2)], 3: [(0, 2), (2, 1)], 4: [(2, 0)]},
         {1: [(1, 2)], 3: [(0, 0)]}]
# by hand: image 0 prototype order 4 (0.9), 0 (0.5), 2 (0.5), 3 (0.2), 1 (0)
#   class 1: 4: 0.9 * 0.1 = 0.09 keep | 0: 0.25 keep | 2: 0.25 keep | 3: 0.2 * 0.04 = 0.008 drop | 1: 0 drop
#   class 2: 4: 0.45 keep | 0, 2: 0 drop | 3: 0.2 * -0.5 = -0.1 keep (abs) | 1: drop
#   class 0: 4: 0 drop | 0: 0.5f * 0.02f < 0.01 drop | 2: 0.005 drop | 3: 0.2 * 0.06 = 0.012 keep | 1: 0 * 1 drop
# image 1 prototype order 1 (1.0), 3 (0.3), 0, 2, 4 (0)
#   class 0: 1: 1.0 keep | 3: 0.3 * 0.06 = 0.018 keep;  class 1: 1: 0 drop | 3: 0.3 * 0.04 = 0.012 keep
#   class 2: 1: 0 drop | 3: -0.15 keep
EXPECTED = [[(1, [(4, 2, 0), (0, 1, 1), (2, 0, 2)]), (2, [(4, 2, 0), (3, 2, 1)]), (0, [(3, 2, 1)])],
            [(0, [(1, 1, 2), (3, 0, 0)]), (1, [(3, 0, 0)]), (2, [(3, 0, 0)])]]


def _hand_case():
    weight = torch.tensor(WEIGHT, dtype=torch.float32)
    pooled = torch.tensor(POOLED, dtype=torch.float32)
    out = torch.tensor(OUT, dtype=torch.float32)
    proto = torch.zeros(2, 5, 3, 3)
    for i, peaks in enumerate(PEAKS):
        for p, where in peaks.items():
            for h, w in where:
                proto[i, p, h, w] = pooled[i, p]
    return proto, pooled, out, weight


def test_restatement_matches_case_worked_by_hand():
    proto, pooled, out, weight = _hand_case()
    for top, ranks_kept in ((3, 3), (None, 3), (2, 2), (1, 1)):
        for i in range(2):
            got = reference_lists(proto[i:i + 1], pooled[i:i + 1], out[i:i + 1], weight, top)
            want = EXPECTED[i][:ranks_kept]
            assert [(c, [(p, h, w) for p, _, _, _, h, w in e]) for c, _, e in got] == want, (top, i)
            for c, logit, entries in got:
                assert logit == OUT[i][c]
                for p, sim, w, simweight, _, _ in entries:
                    assert sim == float(F(POOLED[i][p])) and w == float(F(WEIGHT[c][p]))
                    assert simweight == float(F(POOLED[i][p])) * float(F(WEIGHT[c][p]))     # a double product
                    assert abs(simweight) > 0.01
    # the boundary pair is dropped because its double product is below 0.01, as worked out above
    assert float(F(0.5)) * float(F(0.02)) < 0.01 < 0.5 * 0.02 + 1e-12


def test_pack_cuts_at_max_entries_and_keeps_the_true_count():
    proto, pooled, out, weight = _hand_case()
    images = [reference_lists(proto[i:i + 1], pooled[i:i + 1], out[i:i + 1], weight, None) for i in range(2)]
    res = pack(images, 2)
    assert res["classes"].tolist() == [[1, 2, 0], [0, 1, 2]]
    assert res["count"].tolist() == [[3, 2, 1], [2, 1, 1]]                  # 3 > max_entries: truncated
    assert res["prototype"].tolist() == [[[4, 0], [4, 3], [3, -1]], [[1, 3], [3, -1], [3, -1]]]
    assert res["h_idx"][0].tolist() == [[2, 1], [2, 2], [2, -1]] and res["w_idx"][0].tolist() == [[0, 1], [0, 1], [1, -1]]
    assert res["simweight"][0, 1, 1] == F(float(F(0.2)) * float(F(-0.5))) and res["simweight"][0, 2, 1] == 0
    assert res["logits"].tolist() == [[3.0, 2.0, 1.0], [2.0, 2.0, 1.0]]
