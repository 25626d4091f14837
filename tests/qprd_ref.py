"""The Python twin of the QP-RD walk (x264 --subme 10, mb_analyse_qp_rd; x264vfw_amd/csrc/qprd.hip.h): a pure function over a cost callback.

libx264 is not among the sources this project was written against; the walk is a recollection, restated here straight from its description and on the
device as a resumable state machine.  tests/test_qprd_cpu.py pins this twin on hand-worked cases, tests/test_gpu_qprd.py the device against it."""


class OutOfRange(ValueError):
    pass


def walk(cost, orig_qp, last_qp, qp_min, qp_max, psy, t8_eligible):
    """cost(q, flip) -> (RD cost of the macroblock coded at quantiser q, with the other transform size when flip; cbp_empty of that encode).
    -> (chosen qp, flip decision, [(q, flip), ..] in the order asked).  Raises OutOfRange if the walk ever asks for a quantiser outside [qp_min, qp_max]: it
    chooses inside the range only.  Two rules see to that where x264's rate control would (it clips every macroblock's quantiser to the range; here AQ clips to
    1 .. 51 only): a macroblock whose own quantiser lies outside is left alone, nothing asked; a last_qp outside is not tried."""
    asked = []

    if not qp_min <= orig_qp <= qp_max:
        return orig_qp, False, asked

    def ask(q, flip=False):
        if not qp_min <= q <= qp_max:
            raise OutOfRange(f"quantiser {q} outside [{qp_min}, {qp_max}]")
        asked.append((q, flip))
        c, e = cost(q, flip)
        return int(c), bool(e)

    origcost, empty = ask(orig_qp)
    bcost, bqp = origcost, orig_qp
    origcbp = not empty
    last_tried = False
    for direction in ((1, -1) if origcbp else (-1,)):
        threshold = 1 if psy else 0
        if (last_qp < orig_qp and direction == -1) or (last_qp > orig_qp and direction == 1):
            threshold += 1
        failures, prevcost, checked_qp, checked_cost = 0, origcost, -1, None
        if direction == -1 and not origcbp:
            q = max(orig_qp - threshold - 1, qp_min)
            checked_cost, empty = ask(q)          # not compared with bcost
            if empty:
                if last_qp > q:
                    last_tried = True
                break
            checked_qp = q
        q = orig_qp + direction
        while qp_min <= q <= qp_max:
            if q == last_qp:
                last_tried = True
            if q == checked_qp:
                c = checked_cost                  # reused, not compared with bcost; `empty` stays that of the encode that ran last
            else:
                c, empty = ask(q)
                if c < bcost:
                    bcost, bqp = c, q
            failures = 0 if c < prevcost else failures + 1          # a tie is a failure
            prevcost = c
            if failures > threshold:
                break
            if direction == 1 and empty:
                break
            q += direction
    if not last_tried and qp_min <= last_qp <= qp_max:
        c, _ = ask(last_qp)
        if c < bcost:
            bcost, bqp = c, last_qp
    flip = False
    if bqp != orig_qp and t8_eligible:
        c, _ = ask(bqp, True)
        flip = not c > bcost
    return bqp, flip, asked


def table_cost(cost, empty, cost_flip):
    """the callback over tables indexed by quantiser (x264gpu_qprd_walk's inputs)"""
    return lambda q, flip: ((cost_flip if flip else cost)[q], empty[q])
