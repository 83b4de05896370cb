// cli_run.hpp -- included by csdr_cli.cpp inside its anonymous namespace: device hand-off between adjacent processes, the I/O threads and the streaming loop run()
// ------------------------------------------------------------------ device hand-off between adjacent csdr processes
// north_star: "the stdin->stdout pipe never round-trips to host between stages ... existing shell pipelines drop in unchanged".  In `csdr a | csdr b` both
// ends of the pipe are this binary, both talk to the same GPU, and the samples a produces are already in HBM: writing them to the pipe costs a D2H copy, two
// pipe copies and an H2D copy per stage.  Instead:
//   * b (the consumer), first thing in main(), listens on an abstract unix socket named after the PIPE it reads (st_dev:st_ino of fd 0 -- both ends of a pipe
//     report the same inode);
//   * a (the producer), just before it would write its first byte, tries to connect to the socket named after fd 1.  No listener (the consumer is some other
//     program, or stdout is no pipe): plain bytes, as ever -- a foreign peer never sees anything but the reference's wire format.  Connected: a sends HELLO with
//     the HIP IPC handle of a ring of NBUF output slots in its device memory; b maps it (hipIpcOpenMemHandle) and answers ACK, or NAK (another device, IPC not
//     available in this container, ...) after which both fall back to bytes;
//   * b decides with one poll() on {stdin, listener}: a connection means hand-off, bytes (or EOF) on stdin mean a producer that writes bytes;
//   * per block a writes its result into a free slot, waits for the kernels (stream-ordered event), sends the token {slot, bytes} over the socket; b copies
//     the slot into its own input buffer device-to-device on its stream and returns the slot as a credit once that copy has run.  End of stream = the socket
//     closes.  The 8-byte "csdr"+int preamble of CSDR_DYNAMIC_BUFSIZE_ON still travels through the pipe itself.
// CSDR_AMD_IPC=0 switches the whole mechanism off; CSDR_AMD_IPC_WAIT_MS (default 250) is how long a producer keeps trying to find a listener that is not there
// yet (a consumer of ours listens within a millisecond of its exec, long before the producer's HIP start-up is over); CSDR_AMD_IPC_VERBOSE=1 prints one line
// per link on stderr.
struct IpcHello { char magic[8]; int version, device; char bus_id[32]; hipIpcMemHandle_t mem; unsigned n_slots, reserved; unsigned long long slot_bytes; };
struct IpcToken { unsigned slot, reserved; unsigned long long bytes; };
const char IPC_MAGIC[8] = {'c', 's', 'd', 'r', 'H', 'B', 'M', '1'};
int g_ipc_listen = -1;                       // consumer side: the listening socket named after stdin's pipe
bool ipc_enabled() { const char *e = getenv("CSDR_AMD_IPC"); return !e || atoi(e) != 0; }
bool ipc_verbose() { const char *e = getenv("CSDR_AMD_IPC_VERBOSE"); return e && atoi(e) != 0; }
bool ipc_pipe_name(int fd, struct sockaddr_un *sa, socklen_t *len)
{
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISFIFO(st.st_mode)) return false;
    memset(sa, 0, sizeof *sa); sa->sun_family = AF_UNIX;
    const int n = snprintf(sa->sun_path + 1, sizeof sa->sun_path - 1, "csdr_amd.pipe.%llx.%llx", (unsigned long long)st.st_dev, (unsigned long long)st.st_ino);
    *len = (socklen_t)(offsetof(struct sockaddr_un, sun_path) + 1 + n);                 // abstract name: leading NUL, no file system entry to clean up
    return true;
}
void ipc_listen_on_stdin()
{
    struct sockaddr_un sa; socklen_t len;
    if (!ipc_enabled() || !ipc_pipe_name(STDIN_FILENO, &sa, &len)) return;
    const int fd = socket(AF_UNIX, SOCK_SEQPACKET | SOCK_CLOEXEC, 0);
    if (fd < 0) return;
    if (bind(fd, (struct sockaddr *)&sa, len) != 0 || listen(fd, 1) != 0) { close(fd); return; }
    g_ipc_listen = fd;
}
// the abstract socket name is predictable (dev:ino of the pipe): only a peer of OUR uid gets the IPC handle / is believed (SO_PEERCRED)
bool ipc_peer_is_ours(int fd)
{
    struct ucred cr; socklen_t len = sizeof cr;
    return getsockopt(fd, SOL_SOCKET, SO_PEERCRED, &cr, &len) == 0 && len == sizeof cr && cr.uid == geteuid();
}
void ipc_device_id(int device, char bus_id[32]) { memset(bus_id, 0, 32); if (hipDeviceGetPCIBusId(bus_id, 32, device) != hipSuccess) bus_id[0] = 0; }

// consumer: blocks until the producer has connected (-> the connected socket, ring mapped) or has started to write bytes / closed the pipe (-> -1).  Once.
struct IpcSource { int fd = -1; char *ring = nullptr; unsigned n_slots = 0; size_t slot_bytes = 0; };
bool g_ipc_source_decided = false; IpcSource g_ipc_source;
IpcSource *ipc_source_decide(int device)
{
    if (g_ipc_source_decided) return g_ipc_source.fd >= 0 ? &g_ipc_source : nullptr;
    g_ipc_source_decided = true;
    if (g_ipc_listen < 0) return nullptr;
    int conn = -1;
    for (;;) {
        struct pollfd pf[2] = {{g_ipc_listen, POLLIN, 0}, {STDIN_FILENO, POLLIN, 0}};
        if (poll(pf, 2, -1) < 0) { if (errno == EINTR) continue; break; }
        if (pf[0].revents & POLLIN) { conn = accept4(g_ipc_listen, nullptr, nullptr, SOCK_CLOEXEC); break; }      // (checked first: a producer of ours connects BEFORE it writes the preamble)
        if (pf[1].revents) break;                                                                                  // bytes, EOF or an error on stdin: a producer that writes bytes
    }
    close(g_ipc_listen); g_ipc_listen = -1;
    if (conn < 0) return nullptr;
    if (!ipc_peer_is_ours(conn)) { close(conn); return nullptr; }
    IpcHello h; int ack = 0;
    char mine[32]; ipc_device_id(device, mine);
    void *ring = nullptr;
    const bool test_nak = getenv("CSDR_AMD_IPC_TEST_NAK") != nullptr;  // (tests: refuse as if the handle could not be opened -- the fallback to bytes after a connection)
    if (recv(conn, &h, sizeof h, 0) == (ssize_t)sizeof h && !test_nak && !memcmp(h.magic, IPC_MAGIC, 8) && h.version == 1 && mine[0] && !strncmp(h.bus_id, mine, 32) &&
        hipIpcOpenMemHandle(&ring, h.mem, hipIpcMemLazyEnablePeerAccess) == hipSuccess) ack = 1;
    else (void)hipGetLastError();
    if (send(conn, &ack, sizeof ack, MSG_NOSIGNAL) != (ssize_t)sizeof ack) ack = 0;
    if (!ack) { if (ipc_verbose()) fprintf(stderr, "csdr %s: device hand-off from the previous process refused (another device, or HIP IPC is not available): bytes through the pipe\n", g_cmd); close(conn); return nullptr; }
    g_ipc_source.fd = conn; g_ipc_source.ring = (char *)ring; g_ipc_source.n_slots = h.n_slots; g_ipc_source.slot_bytes = (size_t)h.slot_bytes;
    if (ipc_verbose()) fprintf(stderr, "csdr %s: input arrives by device hand-off (%u slots of %zu bytes in the previous process's HBM ring)\n", g_cmd, h.n_slots, g_ipc_source.slot_bytes);
    return &g_ipc_source;
}

// producer: -> connected socket after HELLO / ACK, or -1 (bytes).  `ring`: n_slots * slot_bytes of device memory from hipMalloc (the base of the allocation)
int ipc_sink_connect(int device, void *ring, unsigned n_slots, size_t slot_bytes)
{
    struct sockaddr_un sa; socklen_t len;
    if (!ipc_enabled() || !ipc_pipe_name(STDOUT_FILENO, &sa, &len)) return -1;
    long wait_ms = 250; if (const char *e = getenv("CSDR_AMD_IPC_WAIT_MS")) wait_ms = atol(e);
    int fd = -1;
    struct timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {
        fd = socket(AF_UNIX, SOCK_SEQPACKET | SOCK_CLOEXEC, 0);
        if (fd < 0) return -1;
        if (connect(fd, (struct sockaddr *)&sa, len) == 0) break;
        close(fd); fd = -1;
        struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((t1.tv_sec - t0.tv_sec) * 1000 + (t1.tv_nsec - t0.tv_nsec) / 1000000 >= wait_ms) return -1;
        usleep(2000);
    }
    if (!ipc_peer_is_ours(fd)) { close(fd); return -1; }
    IpcHello h; memset(&h, 0, sizeof h);
    memcpy(h.magic, IPC_MAGIC, 8); h.version = 1; h.device = device; ipc_device_id(device, h.bus_id); h.n_slots = n_slots; h.slot_bytes = slot_bytes;
    int ack = 0;
    if (hipIpcGetMemHandle(&h.mem, ring) != hipSuccess) { (void)hipGetLastError(); memset(h.magic, 0, 8); }      // (an invalid HELLO: the consumer answers NAK)
    if (send(fd, &h, sizeof h, MSG_NOSIGNAL) != (ssize_t)sizeof h || recv(fd, &ack, sizeof ack, 0) != (ssize_t)sizeof ack || !ack) {
        if (ipc_verbose()) fprintf(stderr, "csdr %s: device hand-off to the next process refused: bytes through the pipe\n", g_cmd);
        close(fd); return -1;
    }
    if (ipc_verbose()) fprintf(stderr, "csdr %s: output leaves by device hand-off (%u slots of %zu bytes)\n", g_cmd, n_slots, slot_bytes);
    return fd;
}

// ------------------------------------------------------------------ the streaming loop: one or more stages, intermediates in HBM
// Host side = three threads around the GPU work so that read(), PCIe and write() overlap (the reference overlaps them with one process per
// command): a READER fills pinned buffers from stdin, the main thread queues H2D -> kernels -> D2H on the context's stream without waiting,
// a WRITER waits for each block's completion event and writes it to stdout.
// Latency: the reader hands a block on as soon as `min_elems` elements have arrived (the reference's the_bufsize, csdr.c:232-247, 332, rounded up to
// the operator's granule) and only takes more when more is ALREADY waiting in the pipe, up to CSDR_AMD_BLOCK elements: a live 2.4 MS/s or 48 kS/s
// stream moves in the reference's own block sizes (6.8 ms / 21 ms), a file or a fast producer in large blocks.
struct HostBuf { char *p = nullptr; size_t cap = 0, bytes = 0; bool eof = false; hipEvent_t ev = nullptr; bool pending = false;
                 const char *dev = nullptr; int slot = -1; };       // device hand-off: where the block lies in the producer's ring; the slot to give back once it is copied (-1: not the slot's last piece)
struct BufQueue {
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER; pthread_cond_t cv = PTHREAD_COND_INITIALIZER; std::vector<HostBuf *> q;
    void push(HostBuf *b) { pthread_mutex_lock(&mu); q.push_back(b); pthread_cond_signal(&cv); pthread_mutex_unlock(&mu); }
    HostBuf *pop() { pthread_mutex_lock(&mu); while (q.empty()) pthread_cond_wait(&cv, &mu); HostBuf *b = q.front(); q.erase(q.begin()); pthread_mutex_unlock(&mu); return b; }
};
struct IoThreads {
    int device = 0; size_t min_bytes = 0, max_bytes = 0;
    BufQueue free_in, full_in, free_out, full_out;
    IpcSource *src = nullptr; BufQueue copied_in;                    // device hand-off, consumer side: blocks whose device copy is queued (their slots go back as credits)
    int sink_fd = -1; HostBuf *sink_bufs = nullptr;                  // producer side: tokens out, credits back; sink_bufs[slot]
    int n_in_bufs = 0;                                               // how many input buffers circulate (reader -> main -> credit thread -> reader)
    std::atomic<bool> sink_closing{false};                           // the writer has sent its last token and shut the socket down: EOF on the credit side is then the normal end
};

// stdin is a regular file (`csdr ... < file`): one thread's read() copies ~14 GB/s out of the page cache into a pinned buffer -- 7 GS/s of u8 IQ, a third of what
// `cat` and the PCIe link manage (profiles/r4_cli_bench.txt).  The block's bytes are then fetched by CSDR_AMD_READERS threads (default 4) with pread() on disjoint
// slices; the file offset is advanced by hand.  Pipes, sockets and ttys keep the single reader (the kernel serialises them anyway).
struct FileInput { bool regular = false; off_t pos = 0; int threads = 1; };
FileInput g_file_in;
void file_input_init()
{
    struct stat st;
    if (fstat(STDIN_FILENO, &st) != 0 || !S_ISREG(st.st_mode)) return;
    const off_t at = lseek(STDIN_FILENO, 0, SEEK_CUR);
    if (at < 0) return;
    int k = 4; if (const char *e = getenv("CSDR_AMD_READERS")) k = atoi(e);
    if (k < 1) k = 1; if (k > 16) k = 16;
    g_file_in.regular = k > 1; g_file_in.pos = at; g_file_in.threads = k;
}
struct PreadJob { char *dst; size_t len; off_t off; size_t got; int err; };
void pread_all(PreadJob *j)
{
    j->got = 0; j->err = 0;
    while (j->got < j->len) {
        const ssize_t r = pread(STDIN_FILENO, j->dst + j->got, j->len - j->got, j->off + (off_t)j->got);
        if (r < 0) { if (errno == EINTR) continue; j->err = errno; break; }      // an I/O error is not the end of the file: reported by read_file_parallel
        if (r == 0) break;
        j->got += (size_t)r;
    }
}
// helper threads that live as long as the process (started at the first parallel read: a thread per block and slice cost more than it saved at 2-MiB blocks)
struct PreadPool {
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER; pthread_cond_t cv_go = PTHREAD_COND_INITIALIZER, cv_done = PTHREAD_COND_INITIALIZER;
    PreadJob *jobs = nullptr; int n_jobs = 0, next = 0, done = 0; unsigned long gen = 0; int n_threads = 0;
} g_pool;
void *pread_pool_main(void *)
{
    unsigned long seen = 0;
    pthread_mutex_lock(&g_pool.mu);
    for (;;) {
        while (g_pool.gen == seen || g_pool.next >= g_pool.n_jobs) { if (g_pool.gen != seen && g_pool.next >= g_pool.n_jobs) seen = g_pool.gen; pthread_cond_wait(&g_pool.cv_go, &g_pool.mu); }
        PreadJob *j = &g_pool.jobs[g_pool.next++];
        pthread_mutex_unlock(&g_pool.mu);
        pread_all(j);
        pthread_mutex_lock(&g_pool.mu);
        if (++g_pool.done == g_pool.n_jobs) pthread_cond_signal(&g_pool.cv_done);
    }
    return nullptr;
}
// up to max_bytes from the file at g_file_in.pos with several threads; a short slice = the end of the file (what lies behind it in later slices is not used)
void read_file_parallel(char *buf, size_t max_bytes, size_t *got, bool *eof)
{
    const int K = g_file_in.threads;
    PreadJob jobs[16];
    size_t slice = (max_bytes / K + 4095) & ~(size_t)4095; if (slice == 0) slice = max_bytes;
    int n = 0;
    for (size_t at = 0; at < max_bytes && n < K; at += slice, n++) jobs[n] = {buf + at, at + slice <= max_bytes ? slice : max_bytes - at, g_file_in.pos + (off_t)at, 0};
    if (g_pool.n_threads == 0) {                                      // (only this thread starts the pool)
        for (int i = 1; i < K; i++) { pthread_t t; if (pthread_create(&t, nullptr, pread_pool_main, nullptr) == 0) { pthread_detach(t); g_pool.n_threads++; } }
        if (g_pool.n_threads == 0) g_pool.n_threads = -1;             // no helpers: this thread reads every slice
    }
    if (g_pool.n_threads > 0 && n > 1) {
        pthread_mutex_lock(&g_pool.mu);
        g_pool.jobs = jobs; g_pool.n_jobs = n; g_pool.next = 1; g_pool.done = 1; g_pool.gen++;      // slice 0 is this thread's
        pthread_cond_broadcast(&g_pool.cv_go);
        pthread_mutex_unlock(&g_pool.mu);
        pread_all(&jobs[0]);
        pthread_mutex_lock(&g_pool.mu);
        while (g_pool.next < g_pool.n_jobs) {                         // (fewer helpers than slices, or none awake yet: take what is left)
            PreadJob *j = &g_pool.jobs[g_pool.next++];
            pthread_mutex_unlock(&g_pool.mu); pread_all(j); pthread_mutex_lock(&g_pool.mu);
            g_pool.done++;
        }
        while (g_pool.done < g_pool.n_jobs) pthread_cond_wait(&g_pool.cv_done, &g_pool.mu);
        g_pool.n_jobs = 0; g_pool.jobs = nullptr;
        pthread_mutex_unlock(&g_pool.mu);
    } else for (int i = 0; i < n; i++) pread_all(&jobs[i]);
    size_t have = 0; bool end = false;
    for (int i = 0; i < n && !end; i++) {
        have += jobs[i].got;
        if (jobs[i].err) {                                            // not an end of file: say so and fail, instead of a silently truncated stream with exit status 0
            fprintf(stderr, "csdr %s: read error on stdin at offset %lld (%s)\n", g_cmd, (long long)(jobs[i].off + (off_t)jobs[i].got), strerror(jobs[i].err));
            exit(5);
        }
        if (jobs[i].got < jobs[i].len) end = true;
    }
    g_file_in.pos += (off_t)have;
    (void)lseek(STDIN_FILENO, g_file_in.pos, SEEK_SET);               // (a later plain read() -- another command sharing the descriptor -- continues behind what was taken)
    *got = have; *eof = end;
}

// blocks until min_bytes have arrived (or EOF / error), then keeps reading only while more is immediately available
void read_some(char *buf, size_t min_bytes, size_t max_bytes, size_t *got, bool *eof)
{
    if (g_file_in.regular && max_bytes >= ((size_t)4 << 20)) { read_file_parallel(buf, max_bytes, got, eof); return; }
    size_t have = 0; *eof = false;
    while (have < max_bytes) {
        if (have >= min_bytes) {
            struct pollfd pf = {STDIN_FILENO, POLLIN, 0};
            if (poll(&pf, 1, 0) <= 0 || !(pf.revents & (POLLIN | POLLHUP))) break;
        }
        ssize_t r = read(STDIN_FILENO, buf + have, max_bytes - have);
        if (r < 0) { if (errno == EINTR) continue; fprintf(stderr, "csdr %s: read error on stdin (%s), treating it as the end of the stream\n", g_cmd, strerror(errno)); *eof = true; break; }
        if (r == 0) { *eof = true; break; }
        have += (size_t)r;
    }
    if (g_file_in.regular) g_file_in.pos += (off_t)have;              // (blocks below 1 MiB take this path on a regular file too)
    *got = have;
}
void *reader_main(void *arg)
{
    IoThreads *io = (IoThreads *)arg;
    (void)hipSetDevice(io->device);
    for (;;) {
        HostBuf *b = io->free_in.pop();
        if (b->pending) { (void)hipEventSynchronize(b->ev); b->pending = false; }      // its previous upload has left the buffer
        read_some(b->p, io->min_bytes, io->max_bytes, &b->bytes, &b->eof);
        const bool eof = b->eof;
        io->full_in.push(b);
        if (eof) return nullptr;
    }
}
void *writer_main(void *arg)
{
    IoThreads *io = (IoThreads *)arg;
    (void)hipSetDevice(io->device);
    for (;;) {
        HostBuf *b = io->full_out.pop();
        if (b->eof) return nullptr;
        if (b->pending) { (void)hipEventSynchronize(b->ev); b->pending = false; }
        if (!write_fully(STDOUT_FILENO, b->p, b->bytes)) _exit(128 + SIGPIPE);      // downstream closed: end quietly, with the status a SIGPIPE death reports to the shell (141)
        io->free_out.push(b);
    }
}

// ---- device hand-off variants of the two I/O threads (+ one thread per direction for the credits)
void *reader_ipc_main(void *arg)
{
    IoThreads *io = (IoThreads *)arg;
    for (;;) {
        IpcToken t;
        const ssize_t r = recv(io->src->fd, &t, sizeof t, 0);
        const bool eof = r != (ssize_t)sizeof t || t.slot >= io->src->n_slots || t.bytes > io->src->slot_bytes;
        if (eof) {
            // The handing-over producer is done.  Whatever any OTHER or later writer of the same pipe sends ( `(csdr a; csdr a2) | csdr b`: a2 finds no listener and
            // writes bytes ) is still part of the stream: carry on in byte mode until stdin itself ends (pinned buffers are only allocated now).
            (void)hipSetDevice(io->device);
            {   // Every block of the ring has been copied out once all input buffers are back (credit_out_main returns a buffer only behind its copy's event):
                // tell the producer so NOW -- it stays alive until we close our side (the ring lives in its memory), and in `(csdr a; csdr a2) | csdr b` the
                // second writer only starts once the first has exited: waiting for stdin's EOF with the socket open would be a deadlock.
                std::vector<HostBuf *> all;
                for (int k = 0; k < io->n_in_bufs; k++) all.push_back(io->free_in.pop());
                shutdown(io->src->fd, SHUT_WR);
                for (HostBuf *b : all) io->free_in.push(b);
            }
            for (;;) {
                HostBuf *b = io->free_in.pop();
                if (b->pending) { (void)hipEventSynchronize(b->ev); b->pending = false; }
                b->dev = nullptr; b->slot = -1;
                if (!b->p && hipHostMalloc((void **)&b->p, b->cap, hipHostMallocDefault) != hipSuccess) { b->p = nullptr; b->bytes = 0; b->eof = true; io->full_in.push(b); return nullptr; }
                read_some(b->p, io->min_bytes, io->max_bytes, &b->bytes, &b->eof);
                const bool end = b->eof;
                io->full_in.push(b);
                if (end) return nullptr;
            }
        }
        size_t off = 0;
        do {                                                         // at most max_bytes per pass, like the byte reader: a token may be cut into several blocks
            HostBuf *b = io->free_in.pop();
            const size_t k = (size_t)t.bytes - off < io->max_bytes ? (size_t)t.bytes - off : io->max_bytes;
            b->dev = io->src->ring + (size_t)t.slot * io->src->slot_bytes + off; b->bytes = k; b->eof = false;
            off += k; b->slot = off == t.bytes ? (int)t.slot : -1;
            io->full_in.push(b);
        } while (off < t.bytes);
    }
}
void *credit_out_main(void *arg)
{   // consumer: a block's device copy has run -> its slot goes back to the producer
    IoThreads *io = (IoThreads *)arg;
    (void)hipSetDevice(io->device);
    for (;;) {
        HostBuf *b = io->copied_in.pop();
        if (b->eof) return nullptr;
        if (b->pending) { (void)hipEventSynchronize(b->ev); b->pending = false; }
        if (b->slot >= 0) { const int s = b->slot; (void)send(io->src->fd, &s, sizeof s, MSG_NOSIGNAL); }
        io->free_in.push(b);
    }
}
void *writer_ipc_main(void *arg)
{
    IoThreads *io = (IoThreads *)arg;
    (void)hipSetDevice(io->device);
    for (;;) {
        HostBuf *b = io->full_out.pop();
        if (b->eof) {
            // the last token is out: close OUR end of the pipe too, now -- the consumer carries on reading bytes from stdin after the hand-off's end (another writer of the
            // same pipe may follow), and without this it saw stdin's EOF only when this process had torn its HIP context down: the seven tear-downs of the README.md:66
            // pipeline ran one after the other (+0.3 s per run, tools/bench_cli.sh)
            // (descriptor 1 stays OCCUPIED -- /dev/null dup2'ed onto it: a bare close() would hand the number to the next open() / socket() of the runtime's tear-down,
            //  and a late write to stdout would land in an unrelated file: ADVICE r5)
            io->sink_closing.store(true); shutdown(io->sink_fd, SHUT_WR);
            { const int nul = open("/dev/null", O_WRONLY); if (nul >= 0) { (void)dup2(nul, STDOUT_FILENO); if (nul != STDOUT_FILENO) (void)close(nul); } else (void)close(STDOUT_FILENO); }
            return nullptr;
        }
        if (b->pending) { (void)hipEventSynchronize(b->ev); b->pending = false; }          // the kernels that filled the slot have run
        IpcToken t = {(unsigned)b->slot, 0u, (unsigned long long)b->bytes};
        if (send(io->sink_fd, &t, sizeof t, MSG_NOSIGNAL) != (ssize_t)sizeof t) _exit(128 + SIGPIPE);   // downstream closed: end quietly, with SIGPIPE's status
    }
}
void *credit_in_main(void *arg)
{   // producer: slots the consumer has copied out
    IoThreads *io = (IoThreads *)arg;
    for (;;) {
        int s = -1;
        const ssize_t r = recv(io->sink_fd, &s, sizeof s, 0);
        if (r < 0 && errno == EINTR) continue;
        // EOF after our own shutdown: the consumer is done.  EOF BEFORE it: the consumer died or left mid-stream (`| head`, its own error exit) -- with every ring
        // slot in flight the main thread sits in free_out.pop() and the writer has no token left to send, so nobody would ever see EPIPE: end quietly,
        // as SIGPIPE ends a producer that writes bytes.
        if (r == 0 && io->sink_closing.load()) return nullptr;
        if (r != (ssize_t)sizeof s || s < 0) _exit(128 + SIGPIPE);      // (a truncated pipeline does not report success: ADVICE r5)
        io->free_out.push(&io->sink_bufs[s]);
    }
}

struct Link { Stage *s; char *d_in[2] = {nullptr, nullptr}; char *d_stage = nullptr; int cur = 0; size_t cap_b = 0, have_b = 0; };   // byte counts: a pipe carries bytes,
                                                                                                               // the reader picks the element size
int run(csdr_amd_ctx *c, std::vector<Stage *> &stages, std::vector<size_t> &caps, int in_bufsize, int out_bufsize, int device)
{
    const size_t n_st = stages.size();
    file_input_init();                                               // (behind whatever the protocol's preamble has taken from stdin)
    std::vector<Link> L(n_st);
    Stage *first = stages[0], *last = stages[n_st - 1];
    const size_t block = caps[0];
    for (size_t k = 0; k < n_st; k++) {
        L[k].s = stages[k]; L[k].cap_b = (k == 0 ? 2 * block + 64 : caps[k]) * stages[k]->in_elem;      // stage 0: unconsumed tail + one new block
        for (int b = 0; b < 2; b++) { L[k].d_in[b] = (char *)csdr_amd_malloc(c, L[k].cap_b + 256); if (!L[k].d_in[b]) die("device buffers"); }
        if (k) { L[k].d_stage = (char *)csdr_amd_malloc(c, L[k].cap_b + 256); if (!L[k].d_stage) die("device buffers"); }
    }
    const size_t cap_out = last->out_capacity(caps[n_st - 1]) + 64;
    hipStream_t st = (hipStream_t)csdr_amd_ctx_stream(c);
    enum { NBUF = 3 };
    HostBuf hin[NBUF], hout[NBUF + 1];
    IoThreads io; io.device = device;
    size_t min_elems = (size_t)(in_bufsize > 0 ? in_bufsize : 1024);
    if (const char *e = getenv("CSDR_AMD_MIN_READ")) { long v = atol(e); if (v > 0) min_elems = (size_t)v; }
    if (min_elems % first->granule) min_elems += first->granule - min_elems % first->granule;
    if (min_elems > block) min_elems = block;
    io.min_bytes = min_elems * first->in_elem; io.max_bytes = block * first->in_elem;
    // device hand-off with the neighbours in the shell pipeline, where they are this binary too (see above): input side decided by now or here, output side offered here
    io.src = ipc_source_decide(device);
    char *ring_out = nullptr;
    const size_t slot_bytes = (cap_out * last->out_elem + 255) & ~(size_t)255;
    {
        struct stat so;
        if (ipc_enabled() && fstat(STDOUT_FILENO, &so) == 0 && S_ISFIFO(so.st_mode) && hipMalloc((void **)&ring_out, NBUF * slot_bytes) == hipSuccess) {
            io.sink_fd = ipc_sink_connect(device, ring_out, NBUF, slot_bytes);
            if (io.sink_fd < 0) { (void)hipFree(ring_out); ring_out = nullptr; }
        }
    }
    io.sink_bufs = hout;
    if (out_bufsize >= 0) send_bufsize(out_bufsize);                 // csdr.c:375-391, through the pipe itself in either mode (< 0: the command sends none)
    for (int k = 0; k < NBUF; k++) {
        hin[k].cap = io.max_bytes + 64; hout[k].cap = cap_out * last->out_elem; hout[k].slot = k;
        if ((!io.src && hipHostMalloc((void **)&hin[k].p, hin[k].cap, hipHostMallocDefault) != hipSuccess) ||
            (io.sink_fd < 0 && hipHostMalloc((void **)&hout[k].p, hout[k].cap, hipHostMallocDefault) != hipSuccess) ||
            hipEventCreateWithFlags(&hin[k].ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&hout[k].ev, hipEventDisableTiming) != hipSuccess) {
            fprintf(stderr, "csdr %s: cannot allocate pinned host buffers\n", g_cmd); exit(3);
        }
        io.free_in.push(&hin[k]); io.free_out.push(&hout[k]);
    }
    io.n_in_bufs = NBUF;
#ifdef F_SETPIPE_SZ
    (void)fcntl(STDIN_FILENO, F_SETPIPE_SZ, 1 << 20); (void)fcntl(STDOUT_FILENO, F_SETPIPE_SZ, 1 << 20);      // fewer, larger pipe transfers (ignored for files)
#endif
    pthread_t th_r, th_w, th_ci, th_co;
    if (pthread_create(&th_r, nullptr, io.src ? reader_ipc_main : reader_main, &io) || pthread_create(&th_w, nullptr, io.sink_fd >= 0 ? writer_ipc_main : writer_main, &io) ||
        (io.src && pthread_create(&th_co, nullptr, credit_out_main, &io)) || (io.sink_fd >= 0 && pthread_create(&th_ci, nullptr, credit_in_main, &io))) {
        fprintf(stderr, "csdr %s: cannot start the I/O threads\n", g_cmd); exit(3);
    }
    void *d_out = csdr_amd_malloc(c, cap_out * last->out_elem + 256);
    if (!d_out) die("device buffers");
    // After EOF the pass is repeated (a few times at most) while some stage still consumes input: an operator that works through its input in
    // windows (fractional_decimator_ff) leaves a tail shorter than its window, which only the next call takes as the end of the stream.
    int extra_passes = 0, rc = 0;
    bool failed = false;
    // CSDR_AMD_CLI_TIMING=1: wall time per stage (the stream drained around every call: a diagnostic, it serialises the process), printed at the end
    const bool timing = getenv("CSDR_AMD_CLI_TIMING") != nullptr;
    std::vector<double> t_stage(n_st, 0.0); std::vector<size_t> n_stage(n_st, 0);
    for (bool eof = false, again = true; again && !failed;) {
        // a new input buffer only when the first operator cannot take a whole block from what it already holds: an operator that leaves a tail per pass
        // (fir_decimate_cc, fractional_decimator_ff, deemphasis_nfm_ff) otherwise let the carry grow by that tail every pass while full blocks kept arriving
        if (!eof && L[0].have_b < block * first->in_elem) {
            HostBuf *b = io.full_in.pop();
            eof = b->eof;
            Link &l0 = L[0];
            if (l0.have_b + b->bytes > l0.cap_b) { fprintf(stderr, "csdr %s: block of %zu elements is too small for this operator (raise CSDR_AMD_BLOCK)\n", g_cmd, block); rc = 1; break; }
            if (b->bytes) {
                if (hipMemcpyAsync(l0.d_in[l0.cur] + l0.have_b, b->dev ? (const void *)b->dev : (const void *)b->p, b->bytes, b->dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess ||
                    hipEventRecord(b->ev, st) != hipSuccess) die("upload");
                b->pending = true; l0.have_b += b->bytes;
            }
            if (!eof) (io.src ? io.copied_in : io.free_in).push(b);      // (hand-off: the slot goes back once the copy has run)
        }
        bool progressed = false;
        for (Stage *s : stages) if (s->ctl && s->ctl->fd && s->ctl_format()) { float a, b2; if (s->ctl->poll(s->ctl_format(), &a, &b2)) s->retune(c, a, b2); }
        // a pass hands the first operator at most `block` elements (what the operators were sized for); what is left waits for the next pass
        size_t n_in = L[0].have_b / first->in_elem;
        const bool all_of_it = n_in <= block;
        if (!all_of_it) n_in = block;                                 // block is a multiple of the granule
        if (!(eof && all_of_it && first->flush_partial)) n_in -= n_in % first->granule;
        if (n_in == 0 && !(eof && n_st > 1)) { again = !eof; continue; }   // at EOF a chain still flushes what its later stages carry
        const char *d_src = L[0].d_in[L[0].cur];
        long n_out = 0;
        for (size_t k = 0; k < n_st; k++) {
            Stage *s = stages[k];
            void *dst = d_out; size_t dst_cap = cap_out;
            if (k + 1 < n_st) {
                Link &nx = L[k + 1];
                // several element-wise kernels want 16-byte aligned pointers: when the consumer's carry is not a multiple of 16 bytes the
                // producer writes to an aligned staging buffer and the result is appended behind the carry by a device copy
                dst = (nx.have_b % 16 == 0) ? nx.d_in[nx.cur] + nx.have_b : nx.d_stage;
                dst_cap = (nx.cap_b - nx.have_b) / s->out_elem;
                if (nx.have_b % s->out_elem) { fprintf(stderr, "csdr chain: element sizes of \"%s\" and its consumer do not line up\n", g_cmd); failed = true; break; }
            }
            size_t consumed = 0;
            struct timespec tq0, tq1;
            if (timing) { (void)hipStreamSynchronize(st); clock_gettime(CLOCK_MONOTONIC, &tq0); }
            n_out = n_in ? s->process(c, d_src, n_in, dst, dst_cap, &consumed) : 0;
            if (timing) { (void)hipStreamSynchronize(st); clock_gettime(CLOCK_MONOTONIC, &tq1); t_stage[k] += (tq1.tv_sec - tq0.tv_sec) + 1e-9 * (tq1.tv_nsec - tq0.tv_nsec); n_stage[k] += n_in; }
            if (consumed) progressed = true;
            {
                Link &lk = L[k];
                if (consumed * s->in_elem > lk.have_b) consumed = lk.have_b / s->in_elem;
                if (k == 0 && consumed == 0 && lk.have_b >= block * s->in_elem && !eof) {
                    fprintf(stderr, "csdr %s: block of %zu elements is too small for this operator (raise CSDR_AMD_BLOCK)\n", g_cmd, block); failed = true; break; }
                const size_t rest_b = lk.have_b - consumed * s->in_elem;
                if (consumed) {
                    if (rest_b) MUST(csdr_amd_d2d(c, lk.d_in[lk.cur ^ 1], lk.d_in[lk.cur] + consumed * s->in_elem, rest_b));
                    lk.cur ^= 1; lk.have_b = rest_b;
                }
            }
            if (k + 1 == n_st) break;
            Link &nx = L[k + 1];
            if (n_out > 0 && nx.have_b % 16 != 0) MUST(csdr_amd_d2d(c, nx.d_in[nx.cur] + nx.have_b, nx.d_stage, (size_t)n_out * s->out_elem));
            nx.have_b += (n_out > 0 ? (size_t)n_out : 0) * s->out_elem;
            n_in = nx.have_b / stages[k + 1]->in_elem;
            if (!(eof && stages[k + 1]->flush_partial)) n_in -= n_in % stages[k + 1]->granule;
            d_src = nx.d_in[nx.cur];
        }
        if (failed) break;
        if (n_out > 0) {
            HostBuf *ob = io.free_out.pop();
            ob->bytes = (size_t)n_out * last->out_elem;
            if (ob->bytes > ob->cap) { fprintf(stderr, "csdr %s: output block larger than its staging buffer\n", g_cmd); io.free_out.push(ob); failed = true; break; }
            if (hipMemcpyAsync(ring_out ? (void *)(ring_out + (size_t)ob->slot * slot_bytes) : (void *)ob->p, d_out, ob->bytes, ring_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipEventRecord(ob->ev, st) != hipSuccess) die("download");
            ob->pending = true;
            // d_out is reused by the next pass: the download is ordered before the next kernels on the same stream
            io.full_out.push(ob);
        }
        bool leftover = false;
        for (size_t k = 0; k < n_st; k++) if (L[k].have_b) leftover = true;
        again = !eof || (progressed && leftover && extra_passes++ < 4);
    }
    // every exit goes through here: what was queued for the writer is written before the process ends
    if (failed) rc = 1;
    if (timing) for (size_t k = 0; k < n_st; k++) fprintf(stderr, "csdr %s: stage %zu: %.3f s for %zu input elements (%.1f M elements/s)\n", g_cmd, k, t_stage[k], n_stage[k], t_stage[k] > 0 ? n_stage[k] / t_stage[k] / 1e6 : 0.0);
    hout[NBUF].eof = true; io.full_out.push(&hout[NBUF]);
    pthread_join(th_w, nullptr);
    (void)hipStreamSynchronize(st);
    if (io.src) { HostBuf end; end.eof = true; io.copied_in.push(&end); pthread_join(th_co, nullptr); close(io.src->fd); }
    if (io.sink_fd >= 0) pthread_join(th_ci, nullptr);               // the ring lives in this process: stay until the consumer has copied the last slot out (it closes the socket then)
    return rc;
}

int passthrough(bool read_preamble, int send_size)
{   // setbuf / clone / through: plumbing commands pipelines use around the hot path (csdr.c:429-451, 2046-2082)
    int b = read_preamble ? get_bufsize(false) : 0;
    send_bufsize(send_size > 0 ? send_size : b);
    std::vector<char> buf(1 << 20);
    for (;;) { size_t got = 0; bool more = read_full(buf.data(), buf.size(), &got); if (got) write_full(buf.data(), got); if (!more) return 0; }
}
