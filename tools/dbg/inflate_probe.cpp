/*
 * inflate_probe.cpp -- wall time of sambamba's BGZF reader (host/bamio.h: bgzf_in_t::next_batch) over a file of BGZF members, with zlib on the pool's
 * threads or with the batch-inflate hook on ssg_bgzf_inflate: the two sides of tools/dbg/inflate_times.py's comparison on the same members.
 *   inflate_probe <members.bgzf> <threads> <device: 0|1|2> <repeats>      one JSON line per pass; 2: both, alternating (the process keeps its device context)
 */
#include <fcntl.h>
#include <time.h>
#include "../../speedseq_amd/host/bamio.h"
#include "../../include/ssgpu.h"

static double wall() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

int main(int argc, char **argv)
{
	if (argc < 5) { fprintf(stderr, "usage: inflate_probe <members.bgzf> <threads> <device: 0|1|2> <repeats>\n"); return 2; }
	const int threads = atoi(argv[2]), which = atoi(argv[3]), repeats = atoi(argv[4]);
	if (which && ssg_device_count() < 1) { fprintf(stderr, "inflate_probe: no device\n"); return 1; }
	for (int r = 0; r < repeats * (which == 2 ? 2 : 1); ++r) {
		const int device = which == 2 ? (r & 1) : which;
		const int fd = open(argv[1], O_RDONLY); if (fd < 0) { perror(argv[1]); return 1; }
		bgzf_inflate_hook = device ? ssg_bgzf_inflate : 0; bgzf_hook_alloc = ssg_host_alloc; bgzf_hook_free = ssg_host_free;   /* as sambamba installs them */
		const double t0 = wall();
		uint64_t bytes = 0, sum = 0, dev = 0, stored = 0;
		{
			bgzf_in_t in(fd, threads);
			std::vector<uint8_t> buf((size_t)1 << 20);
			for (;;) { const size_t k = in.get(buf.data(), buf.size()); if (!k) break; bytes += k; sum += buf[0] + buf[k - 1]; }
			dev = in.n_dev; stored = in.n_stored;
		}
		const double t1 = wall();
		close(fd);
		printf("{\"device\": %d, \"threads\": %d, \"repeat\": %d, \"wall_s\": %.4f, \"payload_bytes\": %llu, \"members_on_device\": %llu, \"stored_members\": %llu, \"hook_kept\": %s, \"check\": %llu}\n",
		       device, threads, which == 2 ? r >> 1 : r, t1 - t0, (unsigned long long)bytes, (unsigned long long)dev, (unsigned long long)stored, !device || bgzf_inflate_hook ? "true" : "false", (unsigned long long)sum);
		fflush(stdout);
	}
	return 0;
}
