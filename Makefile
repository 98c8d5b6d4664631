# Top-level build: product library + executables (HIP, gfx950), CPU oracle, and the test-only emulation build.
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
CSRC    = speedseq_amd/csrc
HOST    = speedseq_amd/host
KHDRS   = $(wildcard $(CSRC)/*.h) include/ssgpu.h
HOSTHDRS = $(wildcard $(HOST)/*.h) include/ssgpu.h $(CSRC)/ssg_types.h
HIPFLAGS = --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable

all: lib tools oracle emu synth

lib: speedseq_amd/libssgpu.so
# Every object's prerequisites come from the compiler (-MMD): no hand-kept header lists, so no object can be stale against a shared
# declaration (round 3 shipped variant libraries linked from objects of different ages).
# the translation units hipcc compiles (sam_format.cpp is plain C++)
UNITS   = ssgpu_core ssg_dbg ssg_index_build ssg_seed ssg_bgzf ssg_bgzf_deep ssg_bgzf_frame ssg_bgzf_inflate ssg_rec_gather ssg_bam_scan ssg_bam_select ssg_msw_replay ssg_bam ssg_coll ssg_b2f ssg_depth ssg_stats ssg_markdup
HIPOBJS = $(UNITS:%=$(CSRC)/%.o)
HIPSRCS = $(UNITS:%=$(CSRC)/%.cpp)
$(HIPOBJS): $(CSRC)/%.o: $(CSRC)/%.cpp
	$(HIPCC) $(HIPFLAGS) -MMD -MP -x hip -c $< -o $@
$(CSRC)/sam_format.o: $(CSRC)/sam_format.cpp
	$(CXX) -O2 -std=c++17 -fPIC -MMD -MP -c $< -o $@
-include $(wildcard $(CSRC)/*.d)
LIBOBJS = $(HIPOBJS) $(CSRC)/sam_format.o
speedseq_amd/libssgpu.so: $(LIBOBJS)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC $(LIBOBJS) -o $@ -lz -ldl

# instrumented build (device phase counters, tools/dbg/phase.py); never the default library
tune: speedseq_amd/libssgpu_tune.so
speedseq_amd/libssgpu_tune.so: $(LIBOBJS)
	$(MAKE) variant NAME=tune VFLAGS="-DSSG_TUNE -DSSG_C2A_WAVES_PER_SIMD=2"

# bench utility: synthetic reference generator (one kernel launch)
synth: tools/synth/libsynthref.so tools/synth/libsynthreads.so
tools/synth/libsynthref.so: tools/synth/synth_ref.cpp
	$(HIPCC) --offload-arch=gfx950 -O3 -shared -fPIC $< -o $@
# soak utility: interleaved FASTQ records of simulated pairs, one kernel launch per chunk (tools/soak.py --stream)
tools/synth/libsynthreads.so: tools/synth/synth_reads.cpp
	$(HIPCC) --offload-arch=gfx950 -O3 -shared -fPIC $< -o $@

# random 64-byte-line gather probe (the roofline denominator of the FM-index kernels; tools/profile_round.sh runs it)
probe: tools/dbg/gather_probe tools/dbg/valu_probe tools/dbg/libm_probe tools/dbg/inflate_probe
# the BGZF reader's wall time with zlib and with the device inflate hook (tools/dbg/inflate_times.py)
tools/dbg/inflate_probe: tools/dbg/inflate_probe.cpp $(HOSTHDRS) speedseq_amd/libssgpu.so
	$(CXX) -O2 -std=c++17 tools/dbg/inflate_probe.cpp -o $@ -Lspeedseq_amd -lssgpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/../../speedseq_amd'
tools/dbg/libm_probe: tools/dbg/libm_probe.cpp
	$(HIPCC) --offload-arch=gfx950 -O3 -ffp-contract=off $< -o $@
tools/dbg/valu_probe: tools/dbg/valu_probe.cpp
	$(HIPCC) --offload-arch=gfx950 -O3 $< -o $@
tools/dbg/gather_probe: tools/dbg/gather_probe.cpp
	$(HIPCC) --offload-arch=gfx950 -O3 $< -o $@

# the executables speedseq.config names (reference bin/speedseq.config:13-14)
tools: bin/bwa bin/samblaster bin/sambamba bin/bamkit
# the helpers `speedseq realign` runs through $$PYTHON (bin/pyrun), under the names speedseq.config gives them
bin/bamkit: $(HOST)/bamkit_main.cpp $(HOSTHDRS) speedseq_amd/libssgpu.so
	$(CXX) -O2 -std=c++17 $(HOST)/bamkit_main.cpp -o $@ -Lspeedseq_amd -lssgpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/../speedseq_amd'
	for t in bamtofastq bamheadrg bamcleanheader bamlibs; do ln -sf bamkit bin/$$t.py; done
bin/sambamba: $(HOST)/sambamba_main.cpp $(HOSTHDRS) speedseq_amd/libssgpu.so
	$(CXX) -O2 -std=c++17 $(HOST)/sambamba_main.cpp -o $@ -Lspeedseq_amd -lssgpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/../speedseq_amd'
bin/bwa: $(HOST)/bwa_main.cpp $(HOSTHDRS) speedseq_amd/libssgpu.so
	$(CXX) -O2 -std=c++17 $(HOST)/bwa_main.cpp -o $@ -Lspeedseq_amd -lssgpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/../speedseq_amd'
bin/samblaster: $(HOST)/samblaster_main.cpp $(HOSTHDRS) speedseq_amd/libssgpu.so
	$(CXX) -O2 -std=c++17 $(HOST)/samblaster_main.cpp -o $@ -Lspeedseq_amd -lssgpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/../speedseq_amd'

oracle:
	$(MAKE) -C oracle

# host emulation of the HIP execution model: same kernel + host sources, CPU-side tests only
emu: tests/emu/libssgpu_emu.so tests/emu/bwa_emu tests/emu/samblaster_emu tests/emu/sambamba_emu tests/emu/bamkit_emu tests/emu/fq_dump tests/emu/fi_test tests/emu/fi_mt_test tests/emu/scan_test tests/emu/cut_test
tests/emu/fi_mt_test: tools/dbg/fi_mt_test.cpp $(HOST)/fast_inflate.h $(HOST)/fast_inflate_mt.h
	$(CXX) -O2 -std=c++17 tools/dbg/fi_mt_test.cpp -o $@ -lz -lpthread
tests/emu/scan_test: tools/dbg/scan_test.cpp $(HOST)/ranksplit.h $(HOST)/ranks.h $(HOST)/fastq.h
	$(CXX) -O2 -std=c++17 -I$(HOST) tools/dbg/scan_test.cpp -o $@ -lz -lpthread
tests/emu/cut_test: tools/dbg/cut_test.cpp $(HOST)/bamio.h
	$(CXX) -O2 -std=c++17 -Wall tools/dbg/cut_test.cpp -o $@ -lz -lpthread
tests/emu/fi_test: tools/dbg/fi_test.cpp $(HOST)/fast_inflate.h
	$(CXX) -O2 -std=c++17 tools/dbg/fi_test.cpp -o $@ -lz
tests/emu/fq_dump: tools/dbg/fq_dump.cpp $(HOST)/fastq.h $(HOST)/fast_inflate.h
	$(CXX) -O2 -std=c++17 tools/dbg/fq_dump.cpp -o $@ -lz -lpthread
tests/emu/libssgpu_emu.so: $(HIPSRCS) $(CSRC)/sam_format.cpp tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -ffp-contract=off -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		$(HIPSRCS) $(CSRC)/sam_format.cpp tests/emu/emu.cpp -shared -o $@ -lpthread -lz
tests/emu/bwa_emu: $(HOST)/bwa_main.cpp $(HOSTHDRS) tests/emu/libssgpu_emu.so
	$(CXX) -O2 -std=c++17 $(HOST)/bwa_main.cpp -o $@ -Ltests/emu -lssgpu_emu -lz -lpthread -Wl,-rpath,'$$ORIGIN'
tests/emu/samblaster_emu: $(HOST)/samblaster_main.cpp $(HOSTHDRS) tests/emu/libssgpu_emu.so
	$(CXX) -O2 -std=c++17 $(HOST)/samblaster_main.cpp -o $@ -Ltests/emu -lssgpu_emu -lz -lpthread -Wl,-rpath,'$$ORIGIN'

tests/emu/sambamba_emu: $(HOST)/sambamba_main.cpp $(HOSTHDRS) tests/emu/libssgpu_emu.so
	$(CXX) -O2 -std=c++17 $(HOST)/sambamba_main.cpp -o $@ -Ltests/emu -lssgpu_emu -lz -lpthread -Wl,-rpath,'$$ORIGIN'
tests/emu/bamkit_emu: $(HOST)/bamkit_main.cpp $(HOSTHDRS) tests/emu/libssgpu_emu.so
	$(CXX) -O2 -std=c++17 $(HOST)/bamkit_main.cpp -o $@ -Ltests/emu -lssgpu_emu -lz -lpthread -Wl,-rpath,'$$ORIGIN'

# memory safety of the inflate kernel's error paths: the emulated kernel under AddressSanitizer and UndefinedBehaviorSanitizer, fed the malformed members of
# tests/test_bgzf_inflate.py and 2000 seeded mutations (tools/dbg/inflate_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
fuzz-inflate: tests/emu/inflate_fuzz
	tests/emu/inflate_fuzz tests/golden/bgzf_inflate_malformed.bin
tests/emu/inflate_fuzz: tools/dbg/inflate_fuzz.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/inflate_fuzz.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety of the record scan's walks on streams that are not what they should be: the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer
# on 3000 seeded streams (tools/dbg/bam_scan_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
fuzz-bam-scan: tests/emu/bam_scan_fuzz
	tests/emu/bam_scan_fuzz
tests/emu/bam_scan_fuzz: tools/dbg/bam_scan_fuzz.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/bam_scan_fuzz.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety and exactness of the selection behind the scan (k_bam_select.h): the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer on 3000
# seeded streams, region lists and filter programs, every refusal among them, and the .bai reader (host/bamio.h) on seeded truncations and mutations of a real index (tools/dbg/bam_select_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
SELFUZZ_SRCS = $(CSRC)/ssg_bam_select.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp
fuzz-bam-select: tests/emu/bam_select_fuzz
	tests/emu/bam_select_fuzz
tests/emu/bam_select_fuzz: tools/dbg/bam_select_fuzz.cpp $(HOST)/bamio.h $(SELFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/bam_select_fuzz.cpp $(SELFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety of the chained match finder of levels 7-9 (k_bgzf_deep.h): the emulated kernel under AddressSanitizer and UndefinedBehaviorSanitizer on the
# kernel's edge payloads and 3000 seeded ones, every stream inflated with zlib (tools/dbg/deflate_deep_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
DEEPFUZZ_SRCS = $(CSRC)/ssg_bgzf.cpp $(CSRC)/ssg_bgzf_deep.cpp $(CSRC)/ssg_bgzf_frame.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp
fuzz-deflate-deep: tests/emu/deflate_deep_fuzz
	tests/emu/deflate_deep_fuzz
tests/emu/deflate_deep_fuzz: tools/dbg/deflate_deep_fuzz.cpp $(DEEPFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/deflate_deep_fuzz.cpp $(DEEPFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety and exactness of bamtofastq on the device (k_b2f.h): the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer on 3000 seeded
# record streams -- truncated aux areas, sequences that leave their record, an l_qname of 0 and of 255 -- in one to three pushes each; every outcome is SSG_EIO or
# the text of a plain C++ restatement (tools/dbg/b2f_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
B2FFUZZ_SRCS = $(CSRC)/ssg_b2f.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp
fuzz-b2f: tests/emu/b2f_fuzz
	tests/emu/b2f_fuzz
tests/emu/b2f_fuzz: tools/dbg/b2f_fuzz.cpp $(B2FFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/b2f_fuzz.cpp $(B2FFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety and exactness of the coverage stage (k_depth.h): the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer on 3000 seeded record
# streams -- spans and clips, filter programs, quality floors, the LDS tile at several sizes, sequences that leave their record, every refusal; counters, sums and
# text against a plain C++ restatement (tools/dbg/depth_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
DEPTHFUZZ_SRCS = $(CSRC)/ssg_depth.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp
fuzz-depth: tests/emu/depth_fuzz
	tests/emu/depth_fuzz
tests/emu/depth_fuzz: tools/dbg/depth_fuzz.cpp $(DEPTHFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/depth_fuzz.cpp $(DEPTHFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety and exactness of the QC tables (k_stats.h): the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer on 3000 seeded record
# streams -- truncations, l_seq and CIGAR lengths that leave the record, aux areas cut short, tiny spans, tiles and slabs, every refusal; every scalar and table
# against a plain C++ loop (tools/dbg/stats_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
STATSFUZZ_SRCS = $(CSRC)/ssg_stats.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp
fuzz-stats: tests/emu/stats_fuzz
	tests/emu/stats_fuzz
tests/emu/stats_fuzz: tools/dbg/stats_fuzz.cpp $(STATSFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/stats_fuzz.cpp $(STATSFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

# memory safety and exactness of the duplicate decision (k_markdup.h): the emulated kernels under AddressSanitizer and UndefinedBehaviorSanitizer on 3000 seeded record
# streams in one to three chunks, every hash width, a broken record in every seventh, the duplicate bits, the counts and the bytes behind the second pass against a
# plain C++ loop of the rule (tools/dbg/markdup_fuzz.cpp; a stand-alone program for the CPU, not part of `emu')
MARKDUPFUZZ_SRCS = $(CSRC)/ssg_markdup.cpp $(CSRC)/ssg_bam_scan.cpp $(CSRC)/ssg_rec_gather.cpp $(CSRC)/ssg_bgzf_inflate.cpp $(CSRC)/ssg_bgzf_frame.cpp
fuzz-markdup: tests/emu/markdup_fuzz
	tests/emu/markdup_fuzz
tests/emu/markdup_fuzz: tools/dbg/markdup_fuzz.cpp $(MARKDUPFUZZ_SRCS) tests/emu/emu.cpp tests/emu/emu.h $(KHDRS)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSSG_EMU -Itests/emu -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-variable \
		tools/dbg/markdup_fuzz.cpp $(MARKDUPFUZZ_SRCS) tests/emu/emu.cpp -o $@ -lpthread -lz

clean:
	rm -rf build; rm -f speedseq_amd/libssgpu.so speedseq_amd/libssgpu_*.so $(CSRC)/*.d tests/emu/libssgpu_emu.so bin/bwa bin/samblaster bin/sambamba bin/bamkit tests/emu/bwa_emu tests/emu/samblaster_emu tests/emu/sambamba_emu tests/emu/bamkit_emu tests/emu/fq_dump tests/emu/fi_test tests/emu/fi_mt_test tests/emu/scan_test tests/emu/cut_test tests/emu/inflate_fuzz tests/emu/bam_scan_fuzz tests/emu/bam_select_fuzz tests/emu/deflate_deep_fuzz tests/emu/b2f_fuzz tests/emu/depth_fuzz tests/emu/stats_fuzz $(CSRC)/*.o
	$(MAKE) -C oracle clean
.PHONY: all lib tools oracle emu clean variant tune fuzz-inflate fuzz-bam-scan fuzz-bam-select fuzz-deflate-deep fuzz-b2f fuzz-depth fuzz-stats fuzz-markdup

# A/B builds of the device library with other compile-time parameters (bench / tests: SSGPU_LIB=speedseq_amd/libssgpu_$(NAME).so); never the
# default.  The units named in VUNITS (default: all) are compiled with VFLAGS into build/$(NAME)/; the others are the product build's
# objects, which `lib` has just brought up to date against every header they include (-MMD), so no stale object can be linked.
#   make variant NAME=x VFLAGS="-D..."                   all translation units
#   make variant NAME=x VFLAGS="-D..." VUNITS=ssg_seed   only that unit (seconds)
VUNITS ?= $(UNITS)
variant: lib
	mkdir -p build/$(NAME) && rm -f build/$(NAME)/*.o
	for u in $(UNITS); do \
	  case " $(VUNITS) " in *" $$u "*) $(HIPCC) $(HIPFLAGS) $(VFLAGS) -x hip -c $(CSRC)/$$u.cpp -o build/$(NAME)/$$u.o || exit 1;; \
	  *) cp $(CSRC)/$$u.o build/$(NAME)/$$u.o;; esac; done
	cp $(CSRC)/sam_format.o build/$(NAME)/sam_format.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC build/$(NAME)/*.o -o speedseq_amd/libssgpu_$(NAME).so -lz -ldl
	rm -rf build/$(NAME)
