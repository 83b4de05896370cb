// cli_io.hpp -- included by csdr_cli.cpp inside its anonymous namespace: messages, descriptor and buffer helpers, the wire protocol and the control channel
const char *g_cmd = "csdr";
int badsyntax(const char *why) { fprintf(stderr, "csdr %s: %s\n", g_cmd, why); return -1; }              // csdr.c:209-218
[[noreturn]] void die(const char *what) { fprintf(stderr, "csdr %s: %s: %s\n", g_cmd, what, csdr_amd_last_error()); exit(3); }
#define MUST(x) do { long rc__ = (long)(x); if (rc__ < 0) die(#x); } while (0)

size_t block_elems()
{
    const char *e = getenv("CSDR_AMD_BLOCK");
    long v = e ? atol(e) : 4194304;
    if (v < 4096) v = 4096;
    return (size_t)(v / 1024 * 1024);
}

int window_from(const char *s)
{   // libcsdr.c:57-63
    if (!strcmp(s, "BOXCAR")) return CSDR_WINDOW_BOXCAR;
    if (!strcmp(s, "BLACKMAN")) return CSDR_WINDOW_BLACKMAN;
    return CSDR_WINDOW_HAMMING;
}
// the optional window argument at argv[k]; without it the reference's commands say which one they took (`who`: the name they print)
int window_arg(int argc, char **argv, int k, const char *who)
{
    if (argc > k) return window_from(argv[k]);
    fprintf(stderr, "csdr %s: window = HAMMING\n", who);
    return CSDR_WINDOW_HAMMING;
}

// ------------------------------------------------------------------ descriptors, buffers and library objects (the public API only: no common.hpp here)
bool fd_number(const char *s, int *fd) { return sscanf(s, "%d", fd) == 1; }
// a path (file or fifo) or fd:<n>, a descriptor this process was started with; < 0: cannot be opened
int open_spec(const char *spec, int flags) { int fd = -1; if (!strncmp(spec, "fd:", 3)) fd_number(spec + 3, &fd); else fd = open(spec, flags, 0644); return fd; }
// reads until `bytes` have arrived or the stream ends; *err (if given) = errno of the read that failed, 0 at a plain end of stream
size_t read_fully(int fd, void *buf, size_t bytes, int *err = nullptr)
{
    size_t have = 0;
    if (err) *err = 0;
    while (have < bytes) {
        const ssize_t r = read(fd, (char *)buf + have, bytes - have);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0 && err) *err = errno;
        if (r <= 0) break;
        have += (size_t)r;
    }
    return have;
}
// writes all of it; false: the write failed (what that means is the caller's business)
bool write_fully(int fd, const void *buf, size_t bytes)
{
    size_t done = 0;
    while (done < bytes) {
        const ssize_t r = write(fd, (const char *)buf + done, bytes - done);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) return false;
        done += (size_t)r;
    }
    return true;
}
struct Fds : std::vector<int> {      // descriptors that are closed when the command returns (< 0: not open)
    using std::vector<int>::vector;
    ~Fds() { for (int fd : *this) if (fd >= 0) close(fd); }
};

struct PinnedFree { void operator()(void *p) const { (void)hipHostFree(p); } };
template <class T> using Pinned = std::unique_ptr<T, PinnedFree>;                      // pinned host memory
template <class T> Pinned<T> pinned_alloc(size_t bytes, const char *what = "pinned buffers")
{
    void *p = nullptr; if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) die(what); return Pinned<T>((T *)p);
}
struct CtxFree { csdr_amd_ctx *c = nullptr; void operator()(void *p) const { csdr_amd_free(c, p); } };
template <class T> using CtxBuf = std::unique_ptr<T, CtxFree>;                         // device memory of a context (csdr_amd_malloc)
template <class T> CtxBuf<T> ctx_alloc(csdr_amd_ctx *c, size_t bytes, const char *what = "device buffers")
{
    T *p = (T *)csdr_amd_malloc(c, bytes); if (!p) die(what); return CtxBuf<T>(p, CtxFree{c});
}
template <auto Destroy> struct Destroyer { template <class T> void operator()(T *p) const { Destroy(p); } };
template <class T, auto Destroy> using Owned = std::unique_ptr<T, Destroyer<Destroy>>;   // a library object, released by its destroy function

// ------------------------------------------------------------------ wire protocol (csdr.c:325-419)
int g_dynamic = 0, g_fixed = 1024, g_fixed_big = 16384, g_print = 0;
void parse_env()
{   // csdr.c:393-419
    if (const char *e = getenv("CSDR_DYNAMIC_BUFSIZE_ON")) { g_dynamic = !!atoi(e); g_fixed = 0; }
    else if (const char *f = getenv("CSDR_FIXED_BUFSIZE")) g_fixed = g_fixed_big = atoi(f);
    if (const char *e = getenv("CSDR_PRINT_BUFSIZES")) g_print = atoi(e);
}
int unitround(int what) { return what <= 0 ? 4 : ((what - 1) & ~3) + 4; }   // csdr.c:352-358

bool read_full(void *buf, size_t bytes, size_t *got)
{   // blocking read of stdin until `bytes` or EOF; returns false on EOF (with *got possibly > 0)
    int err = 0;
    *got = read_fully(STDIN_FILENO, buf, bytes, &err);
    if (err) fprintf(stderr, "csdr %s: read error on stdin (%s), treating it as the end of the stream\n", g_cmd, strerror(err));
    return *got == bytes;
}
void write_full(const void *buf, size_t bytes)
{
    if (!write_fully(STDOUT_FILENO, buf, bytes)) exit(0);         // downstream closed: end quietly like SIGPIPE would
}
int get_bufsize(bool big)
{   // csdr.c:330-341: in dynamic mode the first 8 bytes of stdin are "csdr" + int
    if (!g_dynamic) return unitround(big ? g_fixed_big : g_fixed);
    int first[2] = {0, 0}; size_t got = 0;
    read_full(first, 8, &got);
    if (got != 8 || memcmp(first, "csdr", 4) != 0) {
        badsyntax("warning! Did not match preamble on the beginning of the stream. You should put \"csdr setbuf <buffer size>\" at the beginning of the chain! Falling back to default buffer size: 1024");
        return 1024;
    }
    if (first[1] <= 0) { badsyntax("warning! Invalid buffer size."); exit(254); }
    if (g_print) fprintf(stderr, "csdr %s: buffer size set to %d\n", g_cmd, unitround(first[1]));
    return unitround(first[1]);
}
void send_bufsize(int size)
{   // csdr.c:375-391
    if (!g_dynamic) return;
    if (g_print) fprintf(stderr, "csdr %s: next process proposed input buffer size is %d\n", g_cmd, size);
    int first[2]; memcpy(first, "csdr", 4); first[1] = size;
    write_full(first, 8);
}

// ------------------------------------------------------------------ control channel (csdr.c:252-323)
// lines of a control channel: feed() appends what a non-blocking read returns, next() hands out the complete lines one at a time (without their newline, valid
// until the following feed()); the incomplete rest waits for more, and a line that fills the buffer without a newline is dropped
struct LineSplitter {
    char buf[1024]; int fill = 0, at = 0;
    bool feed(int fd)
    {
        memmove(buf, buf + at, fill - at); fill -= at; at = 0;
        if (fill >= (int)sizeof(buf) - 1 && !memchr(buf, '\n', fill)) fill = 0;
        const ssize_t r = read(fd, buf + fill, sizeof(buf) - 1 - fill);
        if (r > 0) fill += (int)r;
        return r > 0;
    }
    char *next()
    {
        char *line = buf + at, *nl = (char *)memchr(line, '\n', fill - at);
        if (!nl) return nullptr;
        *nl = 0; at = (int)(nl + 1 - buf);
        return line;
    }
};
struct Control {
    int fd = 0; LineSplitter lines;
    bool open_from(int argc, char **argv)
    {
        if (argc < 4) return false;
        if (!strcmp(argv[2], "--fifo")) { fprintf(stderr, "csdr %s: fifo control mode on\n", g_cmd); fd = open(argv[3], O_RDONLY); }
        else if (!strcmp(argv[2], "--fd")) { if (!fd_number(argv[3], &fd)) return false; fprintf(stderr, "csdr %s: fd control mode on, fd=%d\n", g_cmd, fd); }
        else return false;
        if (fd <= 0) { fd = 0; return false; }
        fcntl(fd, F_SETFL, fcntl(fd, F_GETFL, 0) | O_NONBLOCK);
        return true;
    }
    // every complete line is taken, the newest is parsed with the command's scanf format; non-blocking
    bool poll(const char *fmt, float *a, float *b)
    {
        if (!fd || !lines.feed(fd)) return false;
        char *newest = nullptr;
        while (char *l = lines.next()) newest = l;
        float x = 0, y = 0;
        if (!newest || sscanf(newest, fmt, &x, &y) < 1) return false;
        *a = x; *b = y; return true;
    }
    void wait_first(const char *fmt, float *a, float *b) { while (!poll(fmt, a, b)) usleep(10000); }
};

// ------------------------------------------------------------------ command lines as words
// "a b c | d e" -> {{"csdr","a","b","c"},{"csdr","d","e"}}
std::vector<std::vector<std::string>> split_chain(const char *spec)
{
    std::vector<std::vector<std::string>> out(1, std::vector<std::string>(1, "csdr"));
    std::string tok;
    auto flush = [&]() { if (!tok.empty()) { if (tok != "csdr" || out.back().size() > 1) out.back().push_back(tok); tok.clear(); } };
    for (const char *p = spec; *p; p++) {
        if (*p == '|') { flush(); out.push_back(std::vector<std::string>(1, "csdr")); }
        else if (*p == ' ' || *p == '\t' || *p == '\n') flush();
        else tok.push_back(*p);
    }
    flush();
    return out;
}
std::vector<char *> argv_of(std::vector<std::string> &words) { std::vector<char *> av; for (auto &w : words) av.push_back(const_cast<char *>(w.c_str())); return av; }
