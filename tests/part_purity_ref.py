"""Plain-Python restatement of the part-purity evaluation of util/eval_cub_csv.py:57-175 on rows.

It keeps the reference's data structure -- per prototype an insertion-ordered dict from part id to
the list of 0/1 flags, one per row in which the part is visible, with the left member of a pair
folded into the right one and its key removed after every row -- and walks that dict for the tie
rules and the logged tuple.  It deliberately does not use the (n, hits, first_key) reduction the
kernels accumulate: the tests compare that reduction against this."""
from __future__ import annotations

import numpy as np

PATCH = 32


def name_pairs(part_ids, part_names):
    """[(left id, right id)] in file order; KeyError when a left name has no right partner."""
    by_name = dict(zip(part_names, part_ids))
    return [(pid, by_name[name.replace("left", "right")]) for pid, name in zip(part_ids, part_names) if "left" in name]


def _centred(lo, hi):
    """A span wider than the patch is cut to its centre (whole pixels off either end)."""
    extra = (hi - lo) - PATCH
    if extra > 0:
        return lo + extra // 2., hi - extra // 2.
    return lo, hi


def presences_from_rows(rows, parts_of_image, sizes, pairs, image_size, centre=True):
    """rows: (prototype key, image index, h_min, h_max, w_min, w_max) in CSV order;
    parts_of_image[i]: {part id: (x, y)} of the visible parts in file order; sizes[i] = (width, height).
    Returns {prototype: {part id: [0/1 per row]}} in insertion order."""
    scale_to = float(image_size)
    table = {}
    for proto, img, h_lo, h_hi, w_lo, w_hi in rows:
        flags = table.setdefault(proto, {})
        width, height = sizes[img]
        h_lo, h_hi, w_lo, w_hi = float(h_lo), float(h_hi), float(w_lo), float(w_hi)
        if centre:
            h_lo, h_hi = _centred(h_lo, h_hi)
            w_lo, w_hi = _centred(w_lo, w_hi)
        top, bottom = (height / scale_to) * h_lo, (height / scale_to) * h_hi
        left, right = (width / scale_to) * w_lo, (width / scale_to) * w_hi
        visible = parts_of_image[img]
        for pid, (x, y) in visible.items():
            flags.setdefault(pid, []).append(1 if (top <= y <= bottom and left <= x <= right) else 0)
        for lid, rid in pairs:
            if lid not in visible:
                continue
            mine = flags[lid][-1]
            if rid in visible:
                if mine > flags[rid][-1]:
                    flags[rid][-1] = mine
            else:
                flags.setdefault(rid, []).append(mine)
            del flags[lid]                  # the left key goes after every row; it is re-created at its next row
    return table


def evaluate_presences(table, id_to_name):
    """Per-prototype results in the table's order and the logged tuple."""
    best, best_part, best_hits, most, most_purity = {}, {}, {}, {}, {}
    related = 0
    for proto, flags in table.items():
        best[proto], most[proto], most_purity[proto] = 0., ("0", 0), 0.
        for pid, seq in flags.items():
            purity = np.mean(seq)
            hits = np.array(seq).sum()
            if purity > best[proto]:
                take = True
            elif purity == best[proto]:
                take = purity == 0. or hits > best_hits[proto]     # purity 0: the last part; else more hits only
            else:
                take = False
            if take:
                best[proto], best_part[proto], best_hits[proto] = purity, id_to_name[pid], hits
            if hits > most[proto][1]:
                most[proto], most_purity[proto] = (pid, hits), purity
        related += best[proto] > 0.5
    a, b = list(best.values()), list(most_purity.values())
    stats = (float(np.mean(a)), float(np.std(a)), float(np.mean(b)), float(np.std(b))) if a else (float("nan"),) * 4
    return dict(presences=table, max_purity={k: float(v) for k, v in best.items()}, max_part=best_part,
                max_sum={k: int(v) for k, v in best_hits.items()},
                most_part={k: (v[0], int(v[1])) for k, v in most.items()},
                most_purity={k: float(v) for k, v in most_purity.items()}, order=list(table.keys()),
                logged=stats + (len(table), int(related)))


def restate(rows, parts_of_image, sizes, part_ids, part_names, image_size, centre=True):
    table = presences_from_rows(rows, parts_of_image, sizes, name_pairs(part_ids, part_names), image_size, centre)
    return evaluate_presences(table, dict(zip(part_ids, part_names)))
