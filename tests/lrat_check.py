"""A strict LRAT checker in plain Python (test infrastructure; judge (b) of tests/proof_trim_cases.py).  It imports nothing
of the project and knows no watch lists, no search and no GPU: a line `id lits 0 hints 0` is accepted when, under the
negation of its literals, the hinted clauses - in the order given - are unit one after the other and the last one is
falsified.

Strict means: ids above the originals', unique and increasing; a hint names an original clause (ids 1 .. n) or an earlier
line; a hinted clause that is satisfied, has two free literals, or is falsified before the last hint rejects the file, and
so does a last hint that is not falsified.  Deletion lines (`id d ...`) are not accepted: the files under test have none."""


class LratError(Exception):
    pass


def parse(text):
    """LRAT text -> [(id, literals, hints)]."""
    lines = []
    for no, raw in enumerate(text.splitlines(), 1):
        tok = raw.split()
        if not tok:
            continue
        try:
            nums = [int(t) for t in tok]
        except ValueError:
            raise LratError(f"line {no}: not a line of integers: {raw!r}")
        if len(nums) < 3 or nums[-1] != 0 or nums[0] <= 0:
            raise LratError(f"line {no}: malformed")
        try:
            z = nums.index(0, 1)
        except ValueError:
            raise LratError(f"line {no}: no end of the clause")
        lits, hints = nums[1:z], nums[z + 1:-1]
        if 0 in hints or any(h < 0 for h in hints):
            raise LratError(f"line {no}: malformed hints")
        lines.append((nums[0], lits, hints))
    return lines


def check(clauses, text):
    """clauses: the formula, a list of lists of DIMACS literals (clause i has id i + 1).  Returns (ids of the originals
    some line hints, the lines as parse() gives them); raises LratError where the file is rejected."""
    db = {i + 1: list(c) for i, c in enumerate(clauses)}
    n = len(db)
    used = set()
    lines = parse(text)
    last_id = n
    for cid, lits, hints in lines:
        if cid <= last_id:
            raise LratError(f"id {cid}: ids must be above the originals', unique and increasing")
        last_id = cid
        val = {}
        for l in lits:
            if val.get(abs(l), -l) != -l:
                raise LratError(f"id {cid}: the clause holds a literal and its negation")
            val[abs(l)] = -l                    # the negated clause
        if not hints:
            raise LratError(f"id {cid}: no hints")
        for k, h in enumerate(hints):
            if h not in db:
                raise LratError(f"id {cid}: hint {h} is neither an original nor an earlier line")
            free = []
            for l in set(db[h]):
                v = val.get(abs(l))
                if v == l:
                    raise LratError(f"id {cid}: hint {h} is satisfied at its turn")
                if v is None:
                    free.append(l)
            if len(free) > 1:
                raise LratError(f"id {cid}: hint {h} has {len(free)} free literals at its turn")
            is_last = k + 1 == len(hints)
            if not free and not is_last:
                raise LratError(f"id {cid}: hint {h} is falsified before the last hint")
            if free and is_last:
                raise LratError(f"id {cid}: the last hint {h} is not falsified")
            if free:
                val[abs(free[0])] = free[0]
            if h <= n:
                used.add(h)
        db[cid] = list(lits)
    return used, lines
