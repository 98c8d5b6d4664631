"""The block cuts of the device's BAM writers (bgzf_cut_blocks, speedseq_amd/host/bamio.h: the sort's final file, `view -f bam' and `merge' on the device) against the
writer whose rule they restate: tools/dbg/cut_test.cpp sends records of the same lengths through bgzf_out_t::record and requires the ISIZE of every member written
to be the difference of two neighbouring cuts -- records of 1 byte, of a block less one, of a block, of a block and one, of four blocks and three, alone and between
small ones; records that end on a block's last byte; more closed blocks than bgzf_out_t holds before it drains; seeded lengths; no record at all -- and, with forced cuts, a writer on which close_block()
is called before those records, force_blk naming the member that begins there."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "emu", "cut_test")


def test_cut_blocks_cuts_as_the_bgzf_writer():
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/emu/cut_test"])   # always: make's dependency check is cheap, a stale binary tests nothing
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-600:]
    assert r.stdout.startswith("cut_test: 618 sequences"), r.stdout
