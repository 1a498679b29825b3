"""Cases, a model and checks for chains of different lengths verified in passes of equal pieces: mp_verify_shuffle_chain_ragged,
mp_verify_shuffle_chain_ragged_dev, mp_set_chain_pieces and mp_chain_ragged_stats.  Shared by tests/test_chain_piece_emu.py (the kernel
bodies under the development emulator, CPU) and tests/test_gpu_chain_piece.py (the gfx950 build) -- same cases, same expectations.

Expected words: for well-formed links coracle.verify_shuffle link by link, computed BEFORE the library is asked; for a malformed lane (a
coordinate that is not reduced) the per-link call mp_verify_shuffle_batch[_keys].  Every call is followed by mp_chain_ragged_stats, which
must say what the Python model below says about the decomposition -- passes, pieces, the widest pass, the bytes the gather launches moved
-- and that the library copied nothing within host memory.

The model (pieces, passes, descriptor rows) restates chain_ragged_take of csrc/capi.hip and the two bodies of
csrc/kernels_chain_pieces.hpp; source_failures() asserts the lines it restates are still there.

Every run_* function takes an engine (_native.Engine) and the coracle module and returns (failure messages, number of checks made)."""
import ctypes
import os
import re

import mp_oracle as po

WHOLE, BINARY = 0, 1
MODES = (WHOLE, BINARY)
MODE_NAMES = {WHOLE: "whole", BINARY: "binary"}
BAD_ARGUMENT, BAD_ENCODING = -3, -1
MN = (2, 3)                                  # 6 cards: the shape of tests/golden/chain_stark_m2_n3_L3_s21.json
LINKS = [5, 1, 2, 7, 4, 1, 3]                # 23 links in 7 chains
WIDE_MN, WIDE_LINKS = (2, 26), [1, 2, 3]     # 52 cards: rows of 6 656 and 6 368 bytes, many waves per row (GPU only)
BLS_LINKS = [3, 1, 2]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mental-poker_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------- the model
def offsets(links):
    off = [0]
    for n in links:
        off.append(off[-1] + n)
    return off


def pieces_of(n, mode):
    """[(first link a, length l)] of a chain of n links, front to back"""
    if mode == WHOLE:
        return [(0, n)]
    out, a = [], 0
    for b in (1 << k for k in range(11, -1, -1)):       # capi.hip: for (uint32_t b = 2048; binary && b; b >>= 1) if (lk[k] & b)
        if n & b:
            out.append((a, b))
            a += b
    return out


def used_mode(links, mode):
    """the cut that is made: BINARY only where it saves passes -- fewer bits set among the links than distinct lengths (capi.hip:
    __builtin_popcount(bits_set) < lengths) --, so never when all chains have one length"""
    bits = 0
    for n in links:
        bits |= n
    return BINARY if mode == BINARY and bin(bits).count("1") < len(set(links)) else WHOLE


def model(links, mode):
    """-> [(l, [(t, a)], [(deck row, proof row)])], the passes in ascending l, their pieces in (t, a) order"""
    off = offsets(links)
    mode = used_mode(links, mode)
    by_len = {}
    for t, n in enumerate(links):
        for a, l in pieces_of(n, mode):
            by_len.setdefault(l, []).append((t, a))
    return [(l, sorted(ps), [(off[t] + t + a, off[t] + a) for t, a in sorted(ps)]) for l, ps in sorted(by_len.items())]


def model_stats(links, mode, deck_bytes, proof_bytes, key_bytes):
    """what mp_chain_ragged_stats says after a call; key_bytes = 0 for a call without keys"""
    passes = model(links, mode)
    moved = sum(len(ps) * ((l + 1) * deck_bytes + l * (proof_bytes + key_bytes)) for l, ps, _ in passes)
    return [len(passes), sum(len(ps) for _, ps, _ in passes), len(links), sum(links), moved, 0, max(len(ps) for _, ps, _ in passes), used_mode(links, mode)]


def staged(links, mode, rows):
    """the model of the gather: `rows` = the caller's table-major rows of proofs (one per link) -> per pass the link-major rows
    [j * G + g]; and back (the scatter): -> the table-major words.  The identity, if the descriptors are right"""
    out = [None] * len(rows)
    for l, ps, desc in model(links, mode):
        G = len(ps)
        stage = [rows[desc[r % G][1] + r // G] for r in range(l * G)]          # dst[row] = src[desc[g].row + j], row = j G + g
        for x, w in enumerate(stage):
            out[desc[x % G][1] + x // G] = w                                   # status[desc[g].proof_row + j] = words[x]
    return out


_RESTATED = [
    ("capi.hip", r"for \(uint32_t b = 2048; binary && b; b >>= 1\)\s*\n\s*if \(lk\[k\] & b\) \{\s*\n\s*put\(k, a, b\);\s*\n\s*a \+= b;"),
    ("capi.hip", r"if \(!binary\) put\(k, 0, lk\[k\]\);"),
    ("capi.hip", r"const bool binary = t->chain_pieces == MP_CHAIN_PIECES_BINARY && \(uint32_t\)__builtin_popcount\(bits_set\) < lengths;"),
    ("capi.hip", r"h\[2 \* i\] = off \+ k \+ a;\s*\n\s*h\[2 \* i \+ 1\] = off \+ a;"),
    ("capi.hip", r"for \(uint32_t l = 1; l < 4096; \+\+l\)\s*\n\s*if \(next\[l\]\) \{"),
    ("kernels_chain_pieces.hpp", r"dst\[row \* w \+ c\] = src\[\(desc\[2 \* \(size_t\)g \+ which\] \+ j\) \* w \+ c\];"),
    ("kernels_chain_pieces.hpp", r"cp_divmod\(row, G, j, g\);"),
    ("kernels_chain_pieces.hpp", r"a\.status\[a\.desc\[2 \* \(\(size_t\)p\[1\] \+ g\) \+ 1\] \+ j\] = a\.words\[x\];"),
    ("kernels_chain_pieces.hpp", r"const uint32_t j = r / G, g = r % G;"),
]


def source_failures():
    fails = []
    for name, pat in _RESTATED:
        if not re.search(pat, open(os.path.join(CSRC, name)).read()):
            fails.append("%s no longer holds the line the model restates: %s" % (name, pat))
    return fails


def edge_failures():
    """LINKS reaches every edge the decompositions have"""
    fails = source_failures()
    off = offsets(LINKS)
    for mode in MODES:
        if staged(LINKS, mode, list(range(off[-1]))) != list(range(off[-1])):
            fails.append("%s: gather and scatter of the model are not inverse to each other" % MODE_NAMES[mode])
        covered = sorted((t, a + j) for l, ps, _ in model(LINKS, mode) for t, a in ps for j in range(l))
        if covered != [(t, j) for t, n in enumerate(LINKS) for j in range(n)]:
            fails.append("%s: the pieces do not cover every link once" % MODE_NAMES[mode])
    w, b = model(LINKS, WHOLE), model(LINKS, BINARY)
    if [l for l, _, _ in w] != [1, 2, 3, 4, 5, 7] or [len(ps) for _, ps, _ in w] != [2, 1, 1, 1, 1, 1]:
        fails.append("whole: no pass of exactly one piece next to a pass of two (%s)" % [(l, len(ps)) for l, ps, _ in w])
    if [(l, ps) for l, ps, _ in b] != [(1, [(0, 4), (1, 0), (3, 6), (5, 0), (6, 2)]), (2, [(2, 0), (3, 4), (6, 0)]), (4, [(0, 0), (3, 0), (4, 0)])]:
        fails.append("binary: passes %s" % [(l, ps) for l, ps, _ in b])
    single = {n: pieces_of(n, BINARY) for n in (1, 2, 4)}
    if any(single[n] != [(0, n)] for n in single) or not all(n in LINKS for n in single):
        fails.append("no table that is a single piece of 1, 2 and 4 links")
    if pieces_of(7, BINARY) != [(0, 4), (4, 2), (6, 1)] or 7 not in LINKS:
        fails.append("no table with the most pieces for its length (7 = 4 + 2 + 1)")
    if len(model(list(range(1, 4096)), BINARY)) != 12 or [l for l, _, _ in model(list(range(2, 11)), BINARY)] != [1, 2, 4, 8]:
        fails.append("binary: 12 passes at the most, 4 for 2 to 10 seats")
    # the cut is made only where it saves passes: never for chains of one length, not for 1 and 2 links (two bits, two lengths), but for
    # 1, 2 and 3 links (two bits, three lengths)
    if [used_mode(v, BINARY) for v in ([6] * 4, [5, 5], [1, 2], [4095] * 2, [1, 2, 3], LINKS)] != [WHOLE, WHOLE, WHOLE, WHOLE, BINARY, BINARY] or \
            used_mode(LINKS, WHOLE) != WHOLE or len(model([6] * 4, BINARY)) != 1:
        fails.append("the rule that keeps chains whole where the cut saves no pass")
    for mode, mdl in ((WHOLE, w), (BINARY, b)):
        rows_d = sorted(r + j for l, _, desc in mdl for r, _ in desc for j in range(l + 1))
        rows_p = sorted(r + j for l, _, desc in mdl for _, r in desc for j in range(l))
        if rows_d[0] != 0 or rows_d[-1] != off[-1] + len(LINKS) - 1 or rows_p != list(range(off[-1])):
            fails.append("%s: the first and the last row of the arrays are not reached" % MODE_NAMES[mode])
    # the deck at a cut is read by two pieces: inner deck 4 of the 7-link table
    t3 = off[3] + 3
    if sum(1 for l, _, desc in b for r, _ in desc if r <= t3 + 4 <= r + l) != 2:
        fails.append("binary: deck 4 of table 3 does not lie in two pieces")
    return fails


# ---------------------------------------------------------------------------------------------------------------- chains
_CHAINS = {}


def chains(coracle, cvn, mn, links, keyed):
    """-> (g0, [dict(pk, decks, proofs, wit)]) as the oracle shuffles them; wit[j] = the oracle's inputs of link j (rho, perm, prover_seed)"""
    m, n = mn
    key = (cvn, m, n, tuple(links), keyed)
    if key not in _CHAINS:
        g0 = coracle.gen_inputs(cvn, m, n, 150)
        out = []
        for t, L in enumerate(links):
            pk = coracle.gen_inputs(cvn, m, n, 160 + t)["pk"] if keyed else g0["pk"]
            decks, proofs, wit = [coracle.gen_inputs(cvn, m, n, 170 + t)["deck"]], [], []
            for j in range(L):
                gi = coracle.gen_inputs(cvn, m, n, 200 + 10 * j + t)
                d, p = coracle.shuffle_and_remask(cvn, m, n, g0["params"], pk, decks[j], gi["rho"], gi["perm"], gi["prover_seed"])
                decks.append(d)
                proofs.append(p)
                wit.append(gi)
            out.append(dict(pk=pk, decks=decks, proofs=proofs, wit=wit))
        _CHAINS[key] = (g0, out)
    g0, out = _CHAINS[key]
    return g0, [dict(pk=c["pk"], decks=list(c["decks"]), proofs=list(c["proofs"]), keys=[c["pk"]] * len(c["proofs"]), wit=c["wit"]) for c in out]


def flat(ch, keyed):
    """table-major: the decks of table 0, then those of table 1, ...; proofs and keys likewise"""
    return (b"".join(b"".join(c["decks"]) for c in ch), b"".join(b"".join(c["proofs"]) for c in ch),
            b"".join(b"".join(c["keys"]) for c in ch) if keyed else None)


_ORACLE = {}


def oracle_words(coracle, cvn, mn, g0, ch):
    """coracle.verify_shuffle link by link (cached per link: most links of most cases are the honest ones)"""
    out = []
    for c in ch:
        for j in range(len(c["proofs"])):
            key = (cvn, mn, c["keys"][j], c["decks"][j], c["decks"][j + 1], c["proofs"][j])
            if key not in _ORACLE:
                _ORACLE[key] = coracle.verify_shuffle(cvn, mn[0], mn[1], g0["params"], c["keys"][j], c["decks"][j], c["decks"][j + 1], c["proofs"][j])
            out.append(_ORACLE[key])
    return out


def per_link_words(table, ch, keyed):
    """the existing per-link call: what a malformed lane is held to"""
    out = []
    for c in ch:
        for j in range(len(c["proofs"])):
            out += (table.verify_shuffle_batch_keys(c["keys"][j], c["decks"][j], c["decks"][j + 1], c["proofs"][j]) if keyed
                    else table.verify_shuffle_batch(c["decks"][j], c["decks"][j + 1], c["proofs"][j]))
    return out


def _stats_check(fails, tag, table, links, mode, keyed):
    want = model_stats(links, mode, table.N * table.cb, table.proof_bytes, table.pb if keyed else 0)
    got = table.chain_ragged_stats()
    if got != want:
        fails.append("%s: mp_chain_ragged_stats %s, the model %s" % (tag, got, want))
    if got[5] != 0:
        fails.append("%s: the library staged %d bytes in host memory" % (tag, got[5]))


def call_host(fails, tag, table, links, ch, keyed, mode):
    table.set_chain_pieces(mode)
    d, p, k = flat(ch, keyed)
    st = table.verify_shuffle_chain_ragged(links, d, p, k)
    _stats_check(fails, "%s, host, %s" % (tag, MODE_NAMES[mode]), table, links, mode, keyed)
    return st


def call_dev(fails, tag, eng, table, links, keyed, mode, torch, device, d_decks, d_proofs, d_keys):
    table.set_chain_pieces(mode)
    total = sum(links)
    st = torch.full((total,), 0x5A5A5A5, dtype=torch.int32, device=device)
    if device != "cpu":
        torch.cuda.synchronize()
    table.verify_shuffle_chain_ragged_dev(links, d_keys.data_ptr() if keyed else None, d_decks.data_ptr(), d_proofs.data_ptr(), st.data_ptr())
    eng.sync()
    _stats_check(fails, "%s, _dev, %s" % (tag, MODE_NAMES[mode]), table, links, mode, keyed)
    return st.cpu().tolist()


def to_dev(torch, device, raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def _table(eng, g0, mn, keyed):
    return eng.table(mn[0], mn[1], g0["params"], None if keyed else g0["pk"])


# ---------------------------------------------------------------------------------------------------------------- honest chains
def run_honest(eng, coracle, keyed, torch=None, device=None):
    """LINKS, honest: 0 everywhere, in both modes, from host buffers and -- with torch -- from device buffers that the PROVER filled: every
    link is proved by mp_shuffle_and_remask_batch[_keys]_dev from the oracle's witnesses, and its d_out_decks row is copied on the device
    into the table-major array the verifier reads"""
    fails = edge_failures()
    g0, ch = chains(coracle, "stark", MN, LINKS, keyed)
    want = oracle_words(coracle, "stark", MN, g0, ch)
    if want != [0] * sum(LINKS):
        fails.append("the oracle refuses its own chains: %s" % want)
    table = _table(eng, g0, MN, keyed)
    for mode in MODES:
        st = call_host(fails, "honest", table, LINKS, ch, keyed, mode)
        if st != want:
            fails.append("honest chains, host, %s: status %s" % (MODE_NAMES[mode], st))
    checks = 4
    if torch is not None:
        off = offsets(LINKS)
        DB, PSZ, N = table.N * table.cb, table.proof_bytes, table.N
        d_decks = torch.zeros(((off[-1] + len(LINKS)) * DB,), dtype=torch.uint8, device=device)
        d_proofs = torch.zeros((off[-1] * PSZ,), dtype=torch.uint8, device=device)
        d_keys = to_dev(torch, device, flat(ch, True)[2] if keyed else b"\0")
        for t, c in enumerate(ch):
            d_decks[(off[t] + t) * DB:(off[t] + t + 1) * DB] = to_dev(torch, device, c["decks"][0])
        for j in range(max(LINKS)):
            idx = [t for t in range(len(LINKS)) if LINKS[t] > j]
            B = len(idx)
            din = torch.cat([d_decks[(off[t] + t + j) * DB:(off[t] + t + j + 1) * DB] for t in idx]).contiguous()
            rho = to_dev(torch, device, b"".join(ch[t]["wit"][j]["rho"] for t in idx))
            perm = torch.tensor([v for t in idx for v in ch[t]["wit"][j]["perm"]], dtype=torch.int32).to(device)
            seeds = to_dev(torch, device, b"".join(ch[t]["wit"][j]["prover_seed"] for t in idx))
            out_d = torch.zeros((B * DB,), dtype=torch.uint8, device=device)
            out_p = torch.zeros((B * PSZ,), dtype=torch.uint8, device=device)
            pst = torch.full((B,), 7, dtype=torch.int32, device=device)
            if device != "cpu":
                torch.cuda.synchronize()
            if keyed:
                kk = to_dev(torch, device, b"".join(ch[t]["pk"] for t in idx))
                table.shuffle_and_remask_batch_keys_dev(B, kk.data_ptr(), din.data_ptr(), rho.data_ptr(), perm.data_ptr(), seeds.data_ptr(),
                                                        out_d.data_ptr(), out_p.data_ptr(), pst.data_ptr())
            else:
                table.shuffle_and_remask_batch_dev(B, din.data_ptr(), rho.data_ptr(), perm.data_ptr(), seeds.data_ptr(), out_d.data_ptr(),
                                                   out_p.data_ptr(), pst.data_ptr())
            eng.sync()
            if pst.cpu().tolist() != [0] * B:
                fails.append("the prover refuses link %d: %s" % (j, pst.cpu().tolist()))
            for i, t in enumerate(idx):      # the prover's own rows, device to device, into the verifier's table-major arrays
                d_decks[(off[t] + t + j + 1) * DB:(off[t] + t + j + 2) * DB] = out_d[i * DB:(i + 1) * DB]
                d_proofs[(off[t] + j) * PSZ:(off[t] + j + 1) * PSZ] = out_p[i * PSZ:(i + 1) * PSZ]
        if device != "cpu":
            torch.cuda.synchronize()
        hd, hp, _ = flat(ch, keyed)
        if bytes(d_decks.cpu().numpy().tobytes()) != hd or bytes(d_proofs.cpu().numpy().tobytes()) != hp:
            fails.append("the device prover's decks or proofs differ from the oracle's")
        for mode in MODES:
            st = call_dev(fails, "honest", eng, table, LINKS, keyed, mode, torch, device, d_decks, d_proofs, d_keys)
            if st != want:
                fails.append("honest chains, _dev, %s: status %s" % (MODE_NAMES[mode], st))
        checks += 5
    table.close()
    return fails, checks


# ---------------------------------------------------------------------------------------------------------------- defects
def _swap(ch, a, b):
    (ta, ja), (tb, jb) = a, b
    ch[ta]["proofs"][ja], ch[tb]["proofs"][jb] = ch[tb]["proofs"][jb], ch[ta]["proofs"][ja]


def defects(coracle, name, keyed):
    """-> (chains, the links that must fail, malformed).  Table 0 is cut 4 + 1, table 3 is cut 4 + 2 + 1 (BINARY)"""
    g0, ch = chains(coracle, "stark", MN, LINKS, keyed)
    malformed = False
    if name == "the last link of a piece, the last link of the last table":
        _swap(ch, (0, 3), (3, 3))
        ch[6]["proofs"][2] = ch[3]["proofs"][2]
        bad = [(0, 3), (3, 3), (6, 2)]
    elif name == "the first link of the next piece, link 0":
        _swap(ch, (0, 4), (3, 4))
        _swap(ch, (0, 0), (3, 0))
        bad = [(0, 0), (0, 4), (3, 0), (3, 4)]
    elif name == "a boundary deck replaced by another valid deck":
        ch[3]["decks"][4] = ch[0]["decks"][4]
        bad = [(3, 3), (3, 4)]
    elif name == "a wrong key on one link":
        assert keyed
        ch[3]["keys"][5] = ch[4]["pk"]
        bad = [(3, 5)]
    elif name == "a coordinate >= p in a boundary deck":
        d = ch[3]["decks"][4]
        ch[3]["decks"][4] = po.CURVES["stark"].p.to_bytes(32, "little") + d[32:]
        bad, malformed = [(3, 3), (3, 4)], True
    else:
        raise KeyError(name)
    return g0, ch, bad, malformed


DEFECTS = ["the last link of a piece, the last link of the last table", "the first link of the next piece, link 0",
           "a boundary deck replaced by another valid deck", "a wrong key on one link", "a coordinate >= p in a boundary deck"]


def run_defect(eng, coracle, name, keyed=True, torch=None, device=None, settings=False):
    """one defect: exactly the affected links fail, with the oracle's word (the per-link call's for a malformed lane), in both modes, from
    host buffers and (with torch) from device buffers; with settings, under sub-chains of 2 links, passes of 1 table and equations of 2
    tables as well"""
    fails = []
    g0, ch, bad, malformed = defects(coracle, name, keyed)
    off = offsets(LINKS)
    table = _table(eng, g0, MN, keyed)
    want = per_link_words(table, ch, keyed) if malformed else oracle_words(coracle, "stark", MN, g0, ch)
    where = sorted(off[t] + j for t, j in bad)
    if [i for i, v in enumerate(want) if v] != where or (malformed and any(want[i] != BAD_ENCODING for i in where)) or \
            (not malformed and any(want[i] <= 0 for i in where)):
        fails.append("%s: the reference fails the links %s with %s, expected the links %s" %
                     (name, [i for i, v in enumerate(want) if v], [v for v in want if v], where))
    names = [eng.check_name(v) for v in want]
    got = {}
    for mode in MODES:
        got[("host", mode)] = call_host(fails, name, table, LINKS, ch, keyed, mode)
    if torch is not None:
        d, p, k = flat(ch, keyed)
        dd, dp, dk = to_dev(torch, device, d), to_dev(torch, device, p), to_dev(torch, device, k if keyed else b"\0")
        for mode in MODES:
            got[("_dev", mode)] = call_dev(fails, name, eng, table, LINKS, keyed, mode, torch, device, dd, dp, dk)
    if settings:
        for label, on, off_ in (("sub-chains of 2 links", lambda: table.set_chain_max_links(2), lambda: table.set_chain_max_links(0)),
                                ("passes of 1 table", lambda: table.set_chain_slice(1), lambda: table.set_chain_slice(0)),
                                ("equations of 2 tables", lambda: table.set_chain_group(2), lambda: table.set_chain_group(0))):
            on()
            try:
                for mode in MODES:
                    got[(label, mode)] = call_host(fails, name + ", " + label, table, LINKS, ch, keyed, mode)
                    if torch is not None:      # (passes of 1 table: mp_verify_shuffle_chain_dev stages every pass once more, between gather and scatter)
                        got[(label + ", _dev", mode)] = call_dev(fails, name + ", " + label, eng, table, LINKS, keyed, mode, torch, device, dd, dp, dk)
            finally:
                off_()
    for (how, mode), st in sorted(got.items()):
        if st != want or [eng.check_name(v) for v in st] != names:
            fails.append("%s, %s, %s: status %s, expected %s" % (name, how, MODE_NAMES[mode], st, want))
    table.close()
    return fails, 1 + 2 * len(got)


def run_equal(eng, coracle, keyed):
    """all lengths equal (first[k] = k * L): tables 0 and 3 cut down to 5 links each, a proof swapped between them at link 3; the ragged
    call, table-major, in both modes against mp_verify_shuffle_chain on the transposed (link-major) arrays"""
    fails = []
    L = 5
    g0, ch = chains(coracle, "stark", MN, LINKS, keyed)
    pair = [dict(pk=c["pk"], decks=c["decks"][:L + 1], proofs=c["proofs"][:L], keys=c["keys"][:L]) for c in (ch[0], ch[3])]
    _swap(pair, (0, 3), (1, 3))
    want = oracle_words(coracle, "stark", MN, g0, pair)
    if [i for i, v in enumerate(want) if v] != [3, L + 3]:
        fails.append("equal lengths: the oracle fails the links %s" % [i for i, v in enumerate(want) if v])
    table = _table(eng, g0, MN, keyed)
    uni = table.verify_shuffle_chain(2, L, b"".join(pair[t]["decks"][j] for j in range(L + 1) for t in range(2)),
                                     b"".join(pair[t]["proofs"][j] for j in range(L) for t in range(2)),
                                     b"".join(pair[t]["keys"][j] for j in range(L) for t in range(2)) if keyed else None)
    uni_tm = [uni[j * 2 + t] for t in range(2) for j in range(L)]
    for mode in MODES:
        st = call_host(fails, "equal lengths", table, [L, L], pair, keyed, mode)
        if st != want or st != uni_tm:
            fails.append("equal lengths, %s: ragged %s, uniform (transposed) %s, oracle %s" % (MODE_NAMES[mode], st, uni_tm, want))
    table.close()
    return fails, 5


# ---------------------------------------------------------------------------------------------------------------- row widths
def run_width(eng, coracle, cvn, mn, links, torch=None, device=None):
    """another row width: the proof of the last link of the last table replaced by that of the first link of the first; both modes"""
    fails = []
    g0, ch = chains(coracle, cvn, mn, links, False)
    ch[-1]["proofs"][-1] = ch[0]["proofs"][0]
    want = oracle_words(coracle, cvn, mn, g0, ch)
    if [i for i, v in enumerate(want) if v] != [sum(links) - 1] or want[-1] <= 0:
        fails.append("%s %s: the oracle says %s" % (cvn, mn, want))
    table = _table(eng, g0, mn, False)
    got = {}
    for mode in MODES:
        got[("host", mode)] = call_host(fails, "%s %s" % (cvn, mn), table, links, ch, False, mode)
    if torch is not None:
        d, p, _ = flat(ch, False)
        dd, dp = to_dev(torch, device, d), to_dev(torch, device, p)
        for mode in MODES:
            got[("_dev", mode)] = call_dev(fails, "%s %s" % (cvn, mn), eng, table, links, False, mode, torch, device, dd, dp, None)
    for (how, mode), st in sorted(got.items()):
        if st != want:
            fails.append("%s %s, %s, %s: status %s, expected %s" % (cvn, mn, how, MODE_NAMES[mode], st, want))
    table.close()
    return fails, 1 + 2 * len(got)


# ---------------------------------------------------------------------------------------------------------------- refusals
def run_refusals(eng, coracle, torch, device):
    """links[t] = 0, links[t] = 4096, null pointers, a keyless table without keys, mode 2: MP_ERR_BAD_ARGUMENT from both forms, the status
    words and the device buffers as they were, the mode and the stats of the last good call as they were"""
    fails, checks = [], 0
    g0, ch = chains(coracle, "stark", MN, [1, 2], True)
    links = [1, 2]
    d, p, k = flat(ch, True)
    total = 3
    keyless = _table(eng, g0, MN, True)
    own = _table(eng, g0, MN, False)
    own.set_chain_pieces(BINARY)
    if own.verify_shuffle_chain_ragged(links, *flat(chains(coracle, "stark", MN, links, False)[1], False)) != [0] * total:
        fails.append("refusals: the good call before them fails")
    stats = own.chain_ragged_stats()
    lib = eng.lib
    arr = lambda v: (ctypes.c_uint32 * len(v))(*v) if v is not None else None      # noqa: E731
    hd, hp, hk = (ctypes.c_uint8 * len(d)).from_buffer_copy(d), (ctypes.c_uint8 * len(p)).from_buffer_copy(p), (ctypes.c_uint8 * len(k)).from_buffer_copy(k)
    hs = (ctypes.c_int32 * 8)(*([7] * 8))
    dd, dp, dk = to_dev(torch, device, d), to_dev(torch, device, p), to_dev(torch, device, k)
    ds = torch.full((8,), 7, dtype=torch.int32, device=device)
    if device != "cpu":
        torch.cuda.synchronize()
    P = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    cases = [("links[t] = 0", keyless, 2, [1, 0], True, True, True, True), ("links[t] = 4096", keyless, 2, [1, 4096], True, True, True, True),
             ("links = NULL", keyless, 2, None, True, True, True, True), ("tables = 0", keyless, 0, [1, 2], True, True, True, True),
             ("decks = NULL", keyless, 2, links, True, False, True, True), ("proofs = NULL", keyless, 2, links, True, True, False, True),
             ("status = NULL", keyless, 2, links, True, True, True, False), ("a keyless table without keys", keyless, 2, links, False, True, True, True),
             ("the same on a table with a key: links[t] = 0", own, 2, [0, 1], False, True, True, True)]
    for name, tb, tables, lk, wk, wd, wp, ws in cases:
        rc_h = lib.mp_verify_shuffle_chain_ragged(tb.h, tables, arr(lk), hk if wk else None, hd if wd else None, hp if wp else None, hs if ws else None)
        rc_d = lib.mp_verify_shuffle_chain_ragged_dev(tb.h, tables, arr(lk), P(dk) if wk else None, P(dd) if wd else None, P(dp) if wp else None,
                                                      P(ds) if ws else None)
        if rc_h != BAD_ARGUMENT or rc_d != BAD_ARGUMENT:
            fails.append("%s: host %d, _dev %d, expected %d" % (name, rc_h, rc_d, BAD_ARGUMENT))
        checks += 2
    if lib.mp_verify_shuffle_chain_ragged_dev(None, 2, arr(links), P(dk), P(dd), P(dp), P(ds)) != BAD_ARGUMENT:
        fails.append("a null table is accepted")
    # the _dev form moves 16 bytes per lane: an array that is not 16-byte aligned is refused (8 bytes into a good one; nothing is read)
    for name, ak, ad, ap in (("keys", 8, 0, 0), ("decks", 0, 8, 0), ("proofs", 0, 0, 8)):
        if lib.mp_verify_shuffle_chain_ragged_dev(keyless.h, 2, arr(links), P(dk) + ak, P(dd) + ad, P(dp) + ap, P(ds)) != BAD_ARGUMENT:
            fails.append("misaligned %s are accepted" % name)
        checks += 1
    if lib.mp_set_chain_pieces(own.h, 2) != BAD_ARGUMENT or lib.mp_set_chain_pieces(own.h, -1) != BAD_ARGUMENT or lib.mp_set_chain_pieces(None, 0) != BAD_ARGUMENT:
        fails.append("mp_set_chain_pieces accepts mode 2, mode -1 or a null table")
    if lib.mp_chain_ragged_stats(own.h, None) != BAD_ARGUMENT or lib.mp_chain_ragged_stats(None, (ctypes.c_uint64 * 8)()) != BAD_ARGUMENT:
        fails.append("mp_chain_ragged_stats accepts a null argument")
    eng.sync()
    if list(hs) != [7] * 8 or ds.cpu().tolist() != [7] * 8:
        fails.append("a refused call wrote status words: host %s, device %s" % (list(hs), ds.cpu().tolist()))
    if bytes(dd.cpu().numpy().tobytes()) != d or bytes(dp.cpu().numpy().tobytes()) != p or bytes(dk.cpu().numpy().tobytes()) != k or \
            bytes(hd) != d or bytes(hp) != p or bytes(hk) != k:
        fails.append("a refused call wrote to its input buffers")
    if own.chain_ragged_stats() != stats or stats[7] != used_mode(links, BINARY) or stats[0] != 2:
        fails.append("a refused call changed the stats or the mode: %s, before %s" % (own.chain_ragged_stats(), stats))
    # the buffers were good ones: the same arguments with the links in order are accepted, and the words written
    st = call_dev(fails, "after the refusals", eng, keyless, links, True, WHOLE, torch, device, dd, dp, dk)
    if st != [0] * total:
        fails.append("after the refusals: status %s" % st)
    keyless.close()
    own.close()
    return fails, checks + 7
