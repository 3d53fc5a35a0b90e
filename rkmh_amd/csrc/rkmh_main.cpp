// rkmh_main.cpp -- the `rkmh` command line on top of librkmh_amd.so (C ABI in include/rkmh_amd.h): main() and the dispatch.
// What each file holds: rkmh_cli.hpp.
//
// Drop-in for the sub-commands of /root/reference/src/rkmh.cpp that sit on the classify/stream hot path:
//   stream / classify   main_stream   (src/rkmh.cpp:584-989; classify forwards to it, :2744-2747)
//   filter              main_filter   (src/rkmh.cpp:996-1424)
//   call                main_call     (src/rkmh.cpp:1455-1904)
//   hash                main_hash     (src/rkmh.cpp:1931-2116)
// Same flags (option tables src/rkmh.cpp:626-650 and :1963-1983), same stdout line formats
// (src/rkmh.cpp:892), but the per-read OpenMP loop is replaced by batches handed to the GPU while a
// second host thread parses the next batch.  Output order = input order (the reference's order is
// nondeterministic under -t > 1, src/rkmh.cpp:893).
#include <cstdlib>
#include <string>

#include "rkmh_cli.hpp"

int main(int argc, char** argv) {
    if (argc <= 1) { print_help(); exit(1); }
    fork_for_fast_exit();
    // The device front end's workers have a stream each; the runtime maps streams onto four hardware queues unless told otherwise,
    // and kernels of two streams on one queue run one after the other -- the long inflate kernels of BGZF jobs above all
    // (profiles/r05_gz.txt: 2.4 of 8 launches overlapped, 4.2 with 16 queues).  Read by the runtime when it starts: set before any HIP call.
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    rk_default_policy(&g_policy);
    if (const char* e = getenv("RKMH_POLICY")) policy_apply(e, "RKMH_POLICY");
    std::string cmd = argv[1];
    if (cmd == "stream") return main_stream(argc, argv);
    if (cmd == "classify") {
        fprintf(stderr, "CLASSIFY COMMAND IS TEMPORARILY UNAVAILABLE: TRY rkmh stream INSTEAD.\n"); // rkmh.cpp:2746
        return main_stream(argc, argv);
    }
    if (cmd == "hash") return main_hash(argc, argv);
    if (cmd == "filter") return main_filter(argc, argv);
    if (cmd == "call") return main_call(argc, argv);
    if (cmd == "sketch") return main_sketch(argc, argv);
    if (cmd == "dist") return main_dist(argc, argv);
    if (cmd == "gather") return main_gather(argc, argv);
    if (cmd == "multigather") return main_multigather(argc, argv);
    if (cmd == "manysearch") return main_manysearch(argc, argv);
    if (cmd == "cluster") return main_cluster(argc, argv);
    if (cmd == "screen") return main_screen(argc, argv);
    if (cmd == "pack") return main_pack(argc, argv);
    if (cmd == "hpv16") return main_hpv16(argc, argv);
    print_help();
    exit(1);
}
