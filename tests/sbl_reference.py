"""Duplicate, discordant and splitter marking of name-grouped SAM lines, written from the statement of semantics only (SURVEY.md
Appendix C and the header comment of oracle/orc_samblaster.c), for the tests to hold the kernels and the oracle to (test
infrastructure).  Plain Python integers, set, dict and sorted; no hash and no packing anywhere: a signature is the unordered pair of
the two end keys (contig, strand, unclipped 5' coordinate), ("orphan", key) for a pair with one mapped end, or None.

Where the written definition does not decide a case, the functions raise instead of choosing:
  Tie        pieces of a read share a query start and the orders of that run do not all give the same marks;
  Undefined  the two primaries of a pair with both ends mapped disagree on 0x2; a line carries both 0x40 and 0x80; a read of a block
             without two primaries would have splitter lines (the definition speaks of "primary + 0x800/0x100 lines").
"""
import itertools
import re
from collections import namedtuple

DUP, DISC, SPLIT = 1, 2, 4                      # the bits of a line: 0x400 goes into FLAG, discordant stream, splitter stream
MAX_SPLIT_COUNT = 16                            # what the project supports of --maxSplitCount

Line = namedtuple("Line", "contig pos flag mapq cigar")          # contig: index into @SQ or -1 for '*'; pos: 1-based POS; cigar: text or '*'
Opt = namedtuple("Opt", "exclude_dups add_mate_tags max_split_count min_non_overlap max_unmapped_bases min_indel_size")
DEFAULTS = Opt(0, 0, 2, 20, 50, 50)


class Tie(Exception):
    pass


class Undefined(Exception):
    pass


# ---- CIGAR sums -----------------------------------------------------------------------------------------------------------------
def cigar_sums(cigar):
    """(leading S|H, trailing S|H, query bases, reference bases) of a CIGAR in the order it is written (reference order)"""
    if cigar == "*":
        return 0, 0, 0, 0
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    assert "".join("%d%s" % x for x in ops) == cigar, cigar
    body = [i for i, (_, op) in enumerate(ops) if op not in "SH"]
    if not body:
        raise ValueError("a CIGAR of clips only: " + cigar)
    lead = sum(n for n, _ in ops[:body[0]])
    trail = sum(n for n, _ in ops[body[-1] + 1:])
    q = sum(n for n, op in ops if op in "MI=X")
    r = sum(n for n, op in ops if op in "MDN=X")
    return lead, trail, q, r


def is_mapped(l):
    return not (l.flag & 0x4) and l.contig >= 0


def is_reverse(l):
    return bool(l.flag & 0x10)


def query_span(l):
    """first and last aligned base of the piece counted on the read as sequenced: a reverse line's CIGAR is written backwards, so its
    query start is the TRAILING clip"""
    lead, trail, q, _ = cigar_sums(l.cigar)
    s = trail if is_reverse(l) else lead
    return s, s + q - 1


def end_key(l):
    """(contig, strand, unclipped 5' coordinate): forward POS - leading S|H, reverse POS + reference bases - 1 + trailing S|H"""
    lead, trail, _, r = cigar_sums(l.cigar)
    return (l.contig, 1, l.pos + r - 1 + trail) if is_reverse(l) else (l.contig, 0, l.pos - lead)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------
def primaries(block):
    """(index of read 1's primary, of read 2's) in a block (the lines of one QNAME), -1 where there is none: the first line
    without 0x100 / 0x800 of each read"""
    r = [-1, -1]
    for i, l in enumerate(block):
        if l.flag & 0x900:
            continue
        if (l.flag & 0xc0) == 0xc0:
            raise Undefined("a primary line with 0x40 and 0x80")
        for e, bit in enumerate((0x40, 0x80)):
            if (l.flag & bit) and r[e] < 0:
                r[e] = i
    return r[0], r[1]


def signature(block):
    r1, r2 = primaries(block)
    if r1 < 0 or r2 < 0:
        return None                               # not a pair: never a duplicate
    ends = [block[r1], block[r2]]
    keys = [end_key(l) for l in ends if is_mapped(l)]
    if len(keys) == 2:
        return ("pair", tuple(sorted(keys)))
    if len(keys) == 1:
        return ("orphan", keys[0])
    return None


class DupSet:
    """the stream-long duplicate set: the first block of a signature is kept, over all calls"""

    def __init__(self):
        self.seen = set()

    def mark(self, sigs):
        out = []
        for s in sigs:
            out.append(1 if s is not None and s in self.seen else 0)
            if s is not None:
                self.seen.add(s)
        return out


def mark_duplicates(blocks, dupset=None):
    return (dupset or DupSet()).mark([signature(b) for b in blocks])


def owner_side(sigs, ordinals):
    """a duplicate iff the same signature exists with a smaller ordinal (None never is)"""
    first = {}
    for s, o in zip(sigs, ordinals):
        if s is not None:
            p = first.get(s)
            if p is None or o < p:
                first[s] = o
    return [1 if s is not None and o > first[s] else 0 for s, o in zip(sigs, ordinals)]


def mate_lines(block):
    """per line the index of the line MC / MQ are read from: the primary of the other read, -1 for a line of neither read or a block
    without two primaries"""
    r1, r2 = primaries(block)
    if r1 < 0 or r2 < 0:
        return [-1] * len(block)
    return [r2 if l.flag & 0x40 else r1 if l.flag & 0x80 else -1 for l in block]


def discordant(block):
    r1, r2 = primaries(block)
    if r1 < 0 or r2 < 0 or not (is_mapped(block[r1]) and is_mapped(block[r2])):
        return False
    if (block[r1].flag ^ block[r2].flag) & 0x2:
        raise Undefined("the primaries disagree on 0x2")
    return not block[r1].flag & 0x2


def _adjacent_ok(L, R, o):
    (ls, le), (rs, re_) = query_span(L), query_span(R)
    overlap = max(0, 1 + min(le, re_) - max(ls, rs))
    if min(le - ls + 1, re_ - rs + 1) - overlap < o.min_non_overlap:
        return False
    desert = rs - le - 1                          # unaligned read bases between the pieces
    if L.contig == R.contig and is_reverse(L) == is_reverse(R):
        # where each piece starts on the reference, walking in the read's direction
        if is_reverse(L):
            ref_gap = (L.pos + cigar_sums(L.cigar)[3] - 1) - (R.pos + cigar_sums(R.cigar)[3] - 1)
        else:
            ref_gap = R.pos - L.pos
        ins = ref_gap - (rs - ls)
        return abs(ins) >= o.min_indel_size and desert - max(ins, 0) <= o.max_unmapped_bases
    return desert <= o.max_unmapped_bases


def _marks_in_order(pieces, o):
    marked = set()
    for (i, L), (j, R) in zip(pieces, pieces[1:]):
        if _adjacent_ok(L, R, o):
            marked |= {i, j}
    return frozenset(marked)


def splitter_lines(block, read_bit, o):
    """indices of the lines of one read (0x40 or 0x80) that go to the splitter stream"""
    if o.max_split_count > MAX_SPLIT_COUNT:
        raise ValueError("maxSplitCount above %d" % MAX_SPLIT_COUNT)
    pieces = [(i, l) for i, l in enumerate(block) if l.flag & read_bit]
    if not 2 <= len(pieces) <= o.max_split_count or not all(is_mapped(l) for _, l in pieces):
        return frozenset()
    pieces.sort(key=lambda x: query_span(x[1])[0])
    runs = [list(g) for _, g in itertools.groupby(pieces, key=lambda x: query_span(x[1])[0])]
    n_orders = 1
    for r in runs:
        for k in range(2, len(r) + 1):
            n_orders *= k
    if n_orders > 50000:
        raise Tie("too many orders to evaluate")
    results = {_marks_in_order([x for r in order for x in r], o) for order in itertools.product(*[list(itertools.permutations(r)) for r in runs])}
    if len(results) > 1:
        raise Tie("%d outcomes over the orders of equal query starts" % len(results))
    return results.pop()


def classify(block, dup, o):
    """(bits per line, mate line per line) of a block, given the duplicate verdict of its pair"""
    r1, r2 = primaries(block)
    paired = r1 >= 0 and r2 >= 0
    d = bool(dup) and paired
    bits = [DUP if d else 0] * len(block)
    if not paired:
        if splitter_lines(block, 0x40, o) | splitter_lines(block, 0x80, o):
            raise Undefined("splitter lines in a block without two primaries")
        return bits, mate_lines(block)
    if not (d and o.exclude_dups):                # --excludeDups keeps duplicate blocks out of both side streams
        if discordant(block):
            bits[r1] |= DISC
            bits[r2] |= DISC
        for i in splitter_lines(block, 0x40, o) | splitter_lines(block, 0x80, o):
            bits[i] |= SPLIT
    return bits, mate_lines(block)


def process(blocks, o, dupset=None):
    """one call over a chunk of blocks: (dup per block, bits per line, mate line per line as an index into all lines of the chunk)"""
    dups = mark_duplicates(blocks, dupset)
    bits, mate, base = [], [], 0
    for b, d in zip(blocks, dups):
        bb, mm = classify(b, d, o)
        bits += bb
        mate += [m + base if m >= 0 else -1 for m in mm]
        base += len(b)
    return dups, bits, mate


def counts(dups, bits):
    """(duplicate pairs, discordant-stream lines, splitter-stream lines, lines)"""
    return sum(dups), sum(1 for b in bits if b & DISC), sum(1 for b in bits if b & SPLIT), len(bits)


def sort_key(l):
    """tid<<32 | (pos+1)<<1 | rev with 0-based pos, unplaced lines last (tid -1 as unsigned 32 bits, position 0)"""
    if l.contig < 0:
        return 0xffffffff << 32 | (1 if is_reverse(l) else 0)
    return l.contig << 32 | l.pos << 1 | (1 if is_reverse(l) else 0)


# ---- the lines of a pair's records ------------------------------------------------------------------------------------------------
Rec = namedtuple("Rec", "main rid pos flag mapq is_rev cigar")    # main: makes a line (an XA entry does not); rid -1 = unmapped; pos 0-based;
#                                                                   flag: the aligner's own bits (0x40 / 0x80, 0x2, 0x800, 0x10000 = secondary); cigar: ((length, op), ...) in MIDSH


def record_lines(read1, read2):
    """the SAM lines of a pair (the records of read 1, then of read 2; main records only), by the FLAG rules of mem_aln2sam and the SAM
    specification: 0x1; 0x4 for an unmapped read and 0x8 for an unmapped mate; an unmapped read with a mapped mate is placed at the mate's
    contig, position and strand and has no CIGAR; 0x10 own strand, 0x20 the mate's (the read's own when the mate is unmapped and the read
    is not); the secondary bit 0x10000 is printed as 0x100; MAPQ of a line without a contig is 0; clips print as S on a read's first line and as
    H on its later ones.  The mate is the other read's first record."""
    out = []
    for mine, other in ((read1, read2), (read2, read1)):
        if not other or not other[0].main or not any(r.main for r in mine):
            raise Undefined("a read without a main record, or whose first record is none")
        m = other[0]
        which = 0
        for r in mine:
            if not r.main:
                continue
            flag = r.flag | 0x1 | (0x4 if r.rid < 0 else 0) | (0x8 if m.rid < 0 else 0)
            rid, pos, rev, cigar, m_rev = r.rid, r.pos, r.is_rev, r.cigar, m.is_rev
            if r.rid < 0 and m.rid >= 0:
                rid, pos, rev, cigar = m.rid, m.pos, m.is_rev, ()
            if m.rid < 0 and r.rid >= 0:
                m_rev = r.is_rev
            flag |= (0x10 if rev else 0) | (0x20 if m_rev else 0)
            flag = (flag & 0xffff) | (0x100 if flag & 0x10000 else 0)
            # a read's first line keeps soft clips, its later lines print every clip as H (mem_aln2sam without -Y); the sums do not tell S from H
            text = "".join("%d%s" % (n, op if op not in "SH" else "H" if which else "S") for n, op in cigar) or "*"
            which += 1
            out.append(Line(rid, pos + 1, flag, r.mapq, text) if rid >= 0 else Line(-1, 0, flag, 0, "*"))
    return out


# ---- SAM text of lines, for the oracle's executable --------------------------------------------------------------------------------
def sam_text(blocks, names=None, read_len=None):
    out = []
    for b, blk in enumerate(blocks):
        for l in blk:
            out.append("\t".join([names[b] if names else "q%d" % b, str(l.flag), "c%d" % l.contig if l.contig >= 0 else "*", str(l.pos), str(l.mapq), l.cigar,
                                  "*", "0", "0", "*", "*"]))
    return "\n".join(out) + "\n"


def sam_header(n_contigs):
    return "".join("@SQ\tSN:c%d\tLN:100000000\n" % i for i in range(n_contigs))
