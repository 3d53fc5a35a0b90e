// rkmh_exit.cpp -- the process side of `rkmh`: leaving fast (fork_for_fast_exit, done_exit, fail_exit), stage timings, the CPUs
// this process may use and the RKMH_* knobs.
#include <fcntl.h>
#include <sched.h>
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>

#include "rkmh_cli.hpp"

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const bool g_timing = getenv("RKMH_TIMING") != nullptr; // stage timings on stderr
void tick(const char* what, double& t0) {
    if (!g_timing) return;
    const double t = now_s();
    fprintf(stderr, "[rkmh timing] %-28s %.3f s\n", what, t - t0);
    t0 = t;
}

// The command returns when its OUTPUT is complete, not when the kernel has finished taking the process apart.  After _exit the
// driver still unpins every page-locked buffer, unmaps the queues and frees the device memory of the process -- 0.2 to 0.7 s that grew
// with the run (profiles/r05_c3_e2e.txt: "the process leaving"), as much as the main loop of a 64 M-read run.  So main() forks before
// anything touches the GPU: the child does the work, and once every byte is written it closes its output descriptors, tells the parent
// its exit status through a pipe and leaves; the parent -- which holds no GPU state at all -- exits with that status at once, and the
// child's teardown runs on behind it.  A child that dies any other way is waited for and its status passed on.  Not under a
// profiler or RKMH_SLOW_EXIT=1 (the orderly way out), nor with RKMH_FORK=0.
static int g_done_fd = -1; // (child) write end of the status pipe
static std::atomic_flag g_told = ATOMIC_FLAG_INIT; // the status byte goes out once: the first thread to leave sends it
static bool first_to_tell() { return g_done_fd >= 0 && !g_told.test_and_set(); }
static void send_status(int status) {
    const unsigned char b = (unsigned char)status;
    if (write(g_done_fd, &b, 1) != 1) {}
}
static void tell_parent(int status) {
    if (!first_to_tell()) return;
    fflush(stdout); fflush(stderr);
    // Standard output a regular file: every byte is in the page cache, the parent may go -- and only then is the file closed: this is
    // the last descriptor of it (the parent closed its copy after the fork), and ext4 starts allocating and writing back a file that
    // was opened with O_TRUNC ("> out.tsv") at its last close (auto_da_alloc): ~0.1 s per GB, 0.45 s of a 100 M-read run's wall
    // clock (profiles/r06_c3_e2e.txt), which no reader of the file waits for.  A pipe or a terminal: closed first, so that a reader
    // sees the end of the stream no later than the command's return.
    struct stat st;
    const bool regular = fstat(1, &st) == 0 && S_ISREG(st.st_mode);
    if (!regular) { close(1); close(2); }
    send_status(status);
    close(g_done_fd);
    if (regular) { close(1); close(2); }
}
// Leaving after an error: flush what there is and go, WITHOUT running static destructors -- a parser or worker thread may still be
// running, and the HIP runtime's exit handlers are not something to run under it.  Nothing is closed here: other threads may still
// write, and a descriptor 1 or 2 closed under them could be handed to an open() of theirs -- _exit closes them all.
[[noreturn]] void fail_exit() {
    fflush(stdout); fflush(stderr);
    if (first_to_tell()) send_status(1);
    _exit(1);
}
[[noreturn]] void die(const char* what) {
    if (what) fprintf(stderr, "rkmh: %s: %s\n", what, rk_last_error());
    else fprintf(stderr, "rkmh: %s\n", rk_last_error());
    fail_exit();
}
// A profiler's tool library has initialised the GPU runtime before main() (a forked child could not use it) and writes its tables
// from an exit handler (so the process must leave through exit()): rocprofv3 / rocprof / roctracer announce themselves through
// ROCP* / HSA_TOOLS_LIB variables or a preloaded library of theirs.  (Any OTHER preloaded library -- a sanitizer, an exec guard --
// is no reason to give up the fast exit: a first form tested LD_PRELOAD alone, and on a machine that preloads a guard library into
// every process the fork never happened.)
extern char** environ;
static bool under_profiler() {
    static const bool yes = [] {
        for (char** e = environ; e && *e; ++e)
            if (strncmp(*e, "ROCP", 4) == 0 || strncmp(*e, "HSA_TOOLS_LIB=", 14) == 0) return true;
        const char* pre = getenv("LD_PRELOAD");
        return pre && (strstr(pre, "rocprof") || strstr(pre, "roctracer") || strstr(pre, "rocsys") || strstr(pre, "omnitrace") || strstr(pre, "omniperf"));
    }();
    return yes;
}
// Leaving after success: only if every byte really reached standard output (a full disk or a closed pipe must not exit 0)
static const double g_loaded_s = now_s(); // (static initialisation: the program and its libraries are loaded)
[[noreturn]] void done_exit() {
    if (g_timing) {
        fprintf(stderr, "[rkmh timing] %-28s %.3f s\n", "since the program was loaded", now_s() - g_loaded_s);
        // (for scripts that bracket the command with `date +%s.%N`: where the wall clock outside the program goes -- before it was loaded or after its last line)
        const double epoch = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        fprintf(stderr, "[rkmh timing] loaded at epoch %.3f, leaving at epoch %.3f\n", epoch - (now_s() - g_loaded_s), epoch);
    }
    const bool bad = fflush(stdout) != 0 || ferror(stdout);
    fflush(stderr);
    if (bad) fprintf(stderr, "rkmh: write error on standard output\n");
    if (getenv("RKMH_SLOW_EXIT") || under_profiler()) exit(bad ? 1 : 0); // profilers (rocprofv3) write their tables from an exit handler
    tell_parent(bad ? 1 : 0);
    _exit(bad ? 1 : 0); // skips the HIP runtime's and the loader's exit handlers (~0.1-0.2 s of a 1 s run)
}

bool env_flag(const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; }
long env_long(const char* name, long dflt, long lo, long hi) { const char* e = getenv(name); if (!e) return dflt; const long v = atol(e); return v < lo || v > hi ? dflt : v; }

int granted_cpus_main() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n < 1) n = (int)std::thread::hardware_concurrency();
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64]; long long per = 0;
        if (fscanf(f, "%63s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
            const long long quota = atoll(q);
            const int c = (int)((quota + per - 1) / per);
            if (c >= 1 && c < n) n = c;
        }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}

static pid_t g_child = -1;
static void forward_signal(int sig) { if (g_child > 0) kill(g_child, sig); }
// see tell_parent: the parent's side.  Returns in the child (and in a process that does not fork); the parent never returns.
void fork_for_fast_exit() {
    if (getenv("RKMH_SLOW_EXIT") || !env_flag("RKMH_FORK", true) || under_profiler()) return;
    int fds[2];
    if (pipe(fds) != 0) return;
    fflush(stdout); fflush(stderr);
    const pid_t pid = fork();
    if (pid < 0) { close(fds[0]); close(fds[1]); return; }
    if (pid == 0) { close(fds[0]); g_done_fd = fds[1]; return; }
    close(fds[1]);
    close(1); // (the parent writes nothing: the child's descriptor is the file's last one -- see tell_parent)
    g_child = pid;
    for (int sig : {SIGINT, SIGTERM, SIGHUP, SIGQUIT, SIGABRT, SIGPIPE}) signal(sig, forward_signal); // (timeout(1), ^C: they mean the worker)
    close(0); // (the child reads standard input, if anyone does)
    unsigned char b = 0;
    ssize_t n;
    while ((n = read(fds[0], &b, 1)) < 0 && errno == EINTR) {}
    if (n == 1) { // the output is complete: the child finishes dying on its own
        if (getenv("RKMH_TIMING")) {
            char line[96];
            const int len = snprintf(line, sizeof line, "[rkmh timing] parent released at epoch %.3f\n", std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count());
            if (len > 0 && write(2, line, (size_t)len) < 0) {}
        }
        _exit((int)b);
    }
    int st = 0;
    while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {}
    if (WIFEXITED(st)) _exit(WEXITSTATUS(st));
    if (WIFSIGNALED(st)) { signal(WTERMSIG(st), SIG_DFL); raise(WTERMSIG(st)); _exit(128 + WTERMSIG(st)); }
    _exit(1);
}
