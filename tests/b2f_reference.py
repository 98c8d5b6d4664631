"""A plain-Python model of `bamtofastq' (the contract of ssg_b2f_push and of `bamkit bamtofastq'): records parsed with struct, one dict of waiting halves, the
output built as bytes.  It shares nothing with the kernels or with bamkit: it is a second reading of the same recollection of hall-lab/bamkit's bamtofastq.py.
Upstream's script itself is not available to compare with -- src/bamkit is an empty submodule in the reference tree -- so this model and the host path of
bin/bamkit are two restatements of its documented behaviour, and the device path is held to both."""
import struct

LETTERS = b"=ACMGRSVTWYHKDBN"
COMPLEMENT = bytes.maketrans(b"ACGTMKRYVBHD", b"TGCAKMYRBVDH")
FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


class Malformed(Exception):
    def __init__(self, offset):
        Exception.__init__(self, "malformed record at offset %d" % offset)
        self.offset = offset


def split_records(stream, first=0):
    """[(offset, body)] of stream[first:]"""
    out, o = [], first
    while o < len(stream):
        bs, = struct.unpack_from("<I", stream, o)
        assert bs >= 32 and o + 4 + bs <= len(stream)
        out.append((o, stream[o + 4:o + 4 + bs]))
        o += 4 + bs
    return out


def read_group(aux):
    """the last RG:Z the host's walk meets: an unknown type, a Z / H without NUL or a B without its five bytes end the walk"""
    rg, p = b"", 0
    while p + 3 <= len(aux):
        tag, ty = aux[p:p + 2], aux[p + 2:p + 3]
        p += 3
        if ty in FIXED:
            p += FIXED[ty]
        elif ty in (b"Z", b"H"):
            q = aux.find(b"\0", p)
            if q < 0:
                break
            if tag == b"RG" and ty == b"Z":
                rg = aux[p:q]
            p = q + 1
        elif ty == b"B":
            if p + 5 > len(aux):
                break
            cnt, = struct.unpack_from("<I", aux, p + 1)
            p += 5 + {b"c": 1, b"C": 1, b"s": 2, b"S": 2}.get(aux[p:p + 1], 4) * cnt
        else:
            break
    return rg


class Half:
    def __init__(self, offset, body):
        _, _, bmn, fnc, l_seq = struct.unpack_from("<iiIIi", body, 0)
        l_qname, n_cigar = bmn & 0xff, fnc & 0xffff
        self.flag, self.size = fnc >> 16, 4 + len(body)
        o = 32 + l_qname + 4 * n_cigar
        if l_seq < 0 or o + (l_seq + 1) // 2 + l_seq > len(body):
            raise Malformed(offset)
        self.name = body[32:32 + max(l_qname - 1, 0)]
        self.hard = any((v & 0xf) == 5 for v in struct.unpack_from("<%dI" % n_cigar, body, 32 + l_qname))
        packed = body[o:o + (l_seq + 1) // 2]
        seq = bytes(LETTERS[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        o += (l_seq + 1) // 2
        q = body[o:o + l_seq]
        qual = b"I" * l_seq if l_seq > 0 and q[0] == 0xff else bytes((v + 33) & 0xff for v in q)
        if self.flag & 0x10:
            seq, qual = seq[::-1].translate(COMPLEMENT), qual[::-1]
        self.seq, self.qual, self.first = seq, qual, bool(self.flag & 0x40)
        self.rg = read_group(body[o + l_seq:])

    def text(self, name, which):
        return b"@" + name + b"/" + which + (b" RG:Z:" + self.rg if self.rg else b"") + b"\n" + self.seq + b"\n+\n" + self.qual + b"\n"


class Model:
    """the state across pushes (and files): push(stream, first) returns (text, records scanned, pairs written)"""

    def __init__(self, rg=(), rename=False):
        self.want = set(x if isinstance(x, bytes) else x.encode() for x in rg)
        self.rename, self.counter, self.waiting = rename, 0, {}

    def push(self, stream, first=0):
        recs = split_records(stream, first)
        halves = [Half(o, body) for o, body in recs]                      # (a malformed record anywhere: nothing of the call is emitted)
        out, pairs = [], 0
        for h in halves:
            if (h.flag & 0x900) or not (h.flag & 1) or h.hard:
                continue
            if self.want and h.rg not in self.want:
                continue
            held = self.waiting.get(h.name)
            if held is None:
                self.waiting[h.name] = h
                continue
            if held.first == h.first:
                continue
            a, b = (h, held) if h.first else (held, h)
            name = b"%d" % self.counter if self.rename else h.name
            out.append(a.text(name, b"1") + b.text(name, b"2"))
            self.counter += 1
            pairs += 1
            del self.waiting[h.name]
        return b"".join(out), len(recs), pairs

    def held(self):
        """(halves held, bytes of their records)"""
        return len(self.waiting), sum(h.size for h in self.waiting.values())


def bam_records(plain):
    """the offset of the first record of an inflated BAM file"""
    l_text, = struct.unpack_from("<i", plain, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", plain, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", plain, o)
        o += 8 + l_name
    return o


def fastq_of_files(plains, rg=(), rename=False):
    """the whole output for inflated BAM files, and the halves left"""
    m = Model(rg, rename)
    out = b"".join(m.push(p, bam_records(p))[0] for p in plains)
    return out, m.held()[0]
