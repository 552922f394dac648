"""ZIP's long entries through units (flate_hip_zip_read with the option "zip_unit_min") on the CPU, stated independently
of moonbit-flate_amd/csrc/zip_units_rule.h: the set L over zip_ref.Index, and the chain of all L entries' units from
the block walks of one_ref.Walk (dynamic headers start units) and stored_ref.Walk (stored headers too) -- the nodes,
where every node links, the units on the path, their slots and history lengths, and g."""
import one_ref
import stored_ref
import zip_ref as ref

W = 32768


def too_large(e):
    return e.size > 0xffffffff or (e.method == 8 and e.comp_size >= 0x7ffe0000)


def form(entries, sel, unit_min):
    """-> (L, fallback, hull): L = [dict(slot, entry, lo, end, size, out)] in chain order with ARCHIVE offsets."""
    chosen = list(sel) if sel is not None else list(range(len(entries)))
    out_off, cands, seen = [0], [], set()
    for j, i in enumerate(chosen):
        e = entries[i]
        ok = e.status == 0 and not too_large(e)
        out_off.append(out_off[-1] + (e.size if ok else 0))
        if unit_min and ok and e.method == 8 and e.comp_size >= unit_min:
            cands.append(dict(slot=j, entry=i, lo=e.data_off, end=e.data_off + e.comp_size, size=e.size, out=out_off[j],
                              dup=i in seen))
            seen.add(i)
    first = [c for c in cands if not c["dup"]]
    L = [c for c in first if not any(o is not c and o["lo"] < c["end"] and c["lo"] < o["end"] for o in first)]
    hull = (min(c["lo"] for c in L), max(c["end"] for c in L)) if L else (0, 0)
    return L, len(cands) - len(L), hull


def walk_units(f, c, hull_hi, stored):
    """The units of L entry c as the probes see them: the stream is read from its first byte up to the hull's end.
    -> [(start bit, end bit, bytes, final)] of the good units, counted from the entry's first byte, and whether the
    walk ended without error."""
    raw = bytes(f[c["lo"]:hull_hi])
    w = stored_ref.Walk(raw, stored=True) if stored else one_ref.Walk(raw)
    units = []
    for k in range(w.n_units):
        last = w.status == ref.OK and k == w.n_units - 1
        units.append((w.unit_bit[k], w.unit_bit[k + 1], w.out_off[k + 1] - w.out_off[k], last))
    return units, w.status == ref.OK


def chain(f, L, hull, stored, decoys=()):
    """The chain over the hull: List A = every good unit's start behind its entry's first (what FIND must find at
    least) and the given decoy bits, List B = the L entries.  -> dict(cand, probes, next, units, g): probes per node
    (ok, final, end_bit, out); next per node; units = [(node, entry, slot, history)] of the path; g."""
    lo0, hi0 = hull
    per_entry = [walk_units(f, c, hi0, stored) for c in L]
    a_bits = set(decoys)
    for c, (units, _) in zip(L, per_entry):
        a_bits.update(8 * (c["lo"] - lo0) + u[0] for u in units[1:])
    cand = sorted(a_bits)
    na, nb = len(cand), len(L)
    end_sink, dead = na + nb, na + nb + 1
    where = {b: i for i, b in enumerate(cand)}
    probe, owner = {}, {}
    for x, (c, (units, ok)) in enumerate(zip(L, per_entry)):
        base = 8 * (c["lo"] - lo0)
        for k, (sb, eb, n, final) in enumerate(units):
            node = na + x if k == 0 else where[base + sb]
            probe[node] = (1, 1 if final else 0, base + eb, n)
            owner[node] = x
        if not units:
            probe[na + x], owner[na + x] = (0, 0, 0, 0), x
    probes, nxt = [], []
    for node in range(na + nb):
        if node not in probe:  # a decoy, or the start of a unit that failed: its probe fails
            b = cand[node] if node < na else None
            x = next((i for i, c in enumerate(L) if b is not None and c["lo"] - lo0 <= b >> 3 < c["end"] - lo0), None)
            probe[node], owner[node] = (0, 0, 0, 0), x
        ok, final, eb, n = probe[node]
        probes.append(probe[node])
        x = owner[node]
        if not ok or x is None:
            nxt.append(dead)
            continue
        x_end = 8 * (L[x]["end"] - lo0)
        if eb > x_end:
            nxt.append(dead)
        elif final:
            nxt.append(na + x + 1 if x + 1 < nb else end_sink)
        elif eb >= x_end or eb not in where:
            nxt.append(dead)
        else:
            nxt.append(where[eb])
    # the path and what it means
    path, node = [], na
    while node < na + nb:
        path.append(node)
        node = nxt[node]
    good = path if node == end_sink else path[:-1]
    units, g, counting, x, rel = [], 0, True, 0, 0
    for node in good:
        if node >= na:
            x, rel = node - na, 0
        units.append((node, x, L[x]["out"] + rel, min(W, rel)))
        rel += probes[node][3]
        if probes[node][1]:
            if counting and rel == L[x]["size"]:
                g += 1
            else:
                counting = False
    return dict(cand=cand, probes=probes, next=nxt, units=units, g=g)


def served(entry_unit, g_disc, bad_unit):
    g = 0
    while g < g_disc and entry_unit[g + 1] <= bad_unit:
        g += 1
    return g
