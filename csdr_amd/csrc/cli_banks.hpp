// cli_banks.hpp -- included by csdr_cli.cpp inside its anonymous namespace: the bank commands (N channels or N streams through one library object)
// ------------------------------------------------------------------ f4: the ddcd topology in one process
// ddcd runs `csdr fastddc_fwd_cc D | nmux` once and one `csdr fastddc_inv_cc --fd <ctl> D` per client (ddcd_old.cpp:238-252, 474-492):
// N processes re-reading the same spectrum.  Here: one forward transform per block and ONE multi-channel inverse call for all clients;
//   csdr fastddc_bank_cc <decimation> <transition_bw> <window> <ctl | -> <out_0> <shift_rate_0> [<out_1> <shift_rate_1> ...]
// out_k: a path (file or fifo) or fd:<n>;  ctl: a fifo path / fd:<n> carrying lines "<channel> <shift_rate>\n" (newest line per poll), or "-".
// Several GPUs (ddcd_old.cpp:238-252): start the SAME command line once per GPU with CSDR_AMD_RANK / CSDR_AMD_WORLD (and CSDR_AMD_DEVICE) set and
// CSDR_AMD_COMM_FILE naming a path all ranks can reach: rank 0 creates the library's RCCL communicator id there, reads the wideband stream from stdin and the control
// channel; every rank owns a block of the channels (csdr_amd_fastddc_bank_create_sharded) and writes only those outputs.  Per batch rank 0 broadcasts a small header
// (blocks, end of stream, retunes) so that all ranks make the same calls.
int run_bank(csdr_amd_ctx *c, int argc, char **argv, size_t block)
{
    if (argc < 8 || (argc - 6) % 2) return badsyntax("usage: fastddc_bank_cc <decimation> <transition_bw> <window> <ctl|-> <out_0> <rate_0> [<out_k> <rate_k> ...]");
    int D = 0; float tbw = 0.05f; sscanf(argv[2], "%d", &D); sscanf(argv[3], "%g", &tbw);
    const int window = window_from(argv[4]);
    const int n_ch = (argc - 6) / 2;
    int rank = 0, world = 1;
    if (const char *e = getenv("CSDR_AMD_WORLD")) world = atoi(e);
    if (const char *e = getenv("CSDR_AMD_RANK")) rank = atoi(e);
    const bool multi = getenv("CSDR_AMD_WORLD") != nullptr;            // (a world of 1 still goes through the communicator: the single-GPU test of this path)
    if (world < 1 || rank < 0 || rank >= world) return badsyntax("CSDR_AMD_RANK / CSDR_AMD_WORLD out of range");
    Control ctl; Fds ctl_fd(1, -1);
    if (rank == 0 && strcmp(argv[5], "-")) { ctl.fd = ctl_fd[0] = open_spec(argv[5], O_RDONLY | O_NONBLOCK); if (ctl.fd <= 0) return badsyntax("cannot open the control channel"); fcntl(ctl.fd, F_SETFL, fcntl(ctl.fd, F_GETFL, 0) | O_NONBLOCK); }
    std::vector<float> rates(n_ch);
    for (int k = 0; k < n_ch; k++) sscanf(argv[7 + 2 * k], "%g", &rates[k]);
    csdr_fastddc_t ddc;
    if (csdr_amd_fastddc_init(&ddc, tbw, D, 0)) return badsyntax("error in fastddc_init()");
    int nb_max = (int)(block / ddc.input_size); if (nb_max < 1) nb_max = 1;
    csdr_amd_comm *comm = nullptr; csdr_amd_fastddc_bank *bank = nullptr;
    int first = 0, count = n_ch;
    if (multi) {
        const char *cf = getenv("CSDR_AMD_COMM_FILE");
        if (!cf && world > 1) return badsyntax("CSDR_AMD_COMM_FILE must name a file every rank can reach");
        // CSDR_AMD_COMM=ipc: the ranks are processes on ONE box joined by unix sockets named after CSDR_AMD_COMM_FILE and HIP IPC (csdr_amd_comm_create_ipc) -- RCCL refuses
        // two ranks per device, so this is how the per-rank bootstrap of this command is exercised on a single GPU (tests/test_cli_gpu.py); default: RCCL over xGMI
        const char *ct = getenv("CSDR_AMD_COMM");
        const bool use_ipc = ct && !strcmp(ct, "ipc");
        char id[128];
        if (use_ipc) {
            if (!cf) return badsyntax("CSDR_AMD_COMM=ipc needs CSDR_AMD_COMM_FILE (the sockets' path prefix)");
            comm = csdr_amd_comm_create_ipc(c, cf, rank, world);
            if (!comm) die("communicator (ipc)");
        } else
        if (rank == 0) {
            if (csdr_amd_comm_unique_id(id)) die("communicator id");
            if (cf) { std::string tmp = std::string(cf) + ".tmp"; FILE *f = fopen(tmp.c_str(), "wb"); if (!f || fwrite(id, 1, 128, f) != 128) die("cannot write CSDR_AMD_COMM_FILE"); fclose(f); if (rename(tmp.c_str(), cf)) die("rename CSDR_AMD_COMM_FILE"); }
        } else {
            bool ok = false;
            for (int tries = 0; tries < 6000 && !ok; tries++) { FILE *f = fopen(cf, "rb"); if (f) { ok = fread(id, 1, 128, f) == 128; fclose(f); } if (!ok) usleep(10000); }
            if (!ok) die("timed out waiting for CSDR_AMD_COMM_FILE");
        }
        if (!use_ipc) comm = csdr_amd_comm_create(c, id, rank, world);
        if (!comm) die("communicator");
        // the schedule: the library's choice for this world size (channel shards up to two ranks, time slices beyond), or CSDR_AMD_SHARD=channels|blocks
        const char *sh = getenv("CSDR_AMD_SHARD");
        const int mode = (sh && !strcmp(sh, "blocks")) ? CSDR_AMD_SHARD_BLOCKS : (sh && !strcmp(sh, "channels")) ? CSDR_AMD_SHARD_CHANNELS : csdr_amd_fastddc_bank_default_shard_mode(world);
        bank = csdr_amd_fastddc_bank_create_sharded_by(c, tbw, D, rates.data(), n_ch, window, nb_max, comm, mode);
        if (bank) fprintf(stderr, "csdr fastddc_bank_cc: rank %d of %d, %s transport, schedule: %s\n", rank, world, use_ipc ? "ipc" : "rccl", mode == CSDR_AMD_SHARD_BLOCKS ? "time slices" : "channel shards");
        if (bank) csdr_amd_fastddc_bank_channel_slice(bank, &first, &count);
    } else bank = csdr_amd_fastddc_bank_create(c, tbw, D, rates.data(), n_ch, window, nb_max);
    if (!bank) die("fastddc_bank create");
    Owned<csdr_amd_comm, csdr_amd_comm_destroy> comm_owner(comm);      // (released behind the bank, on every way out)
    Owned<csdr_amd_fastddc_bank, csdr_amd_fastddc_bank_destroy> bank_owner(bank);
    Fds out_fd(n_ch, -1);
    for (int k = first; k < first + count; k++) {                       // this rank's clients only
        out_fd[k] = open_spec(argv[6 + 2 * k], O_WRONLY | O_CREAT | O_TRUNC);
        if (out_fd[k] < 0) { fprintf(stderr, "csdr fastddc_bank_cc: cannot open output %s\n", argv[6 + 2 * k]); return -1; }
    }
    const size_t pitch = (size_t)csdr_amd_fastddc_bank_max_output(bank, nb_max) + 8;
    const size_t in_elems = (size_t)nb_max * ddc.input_size;
    const auto h_in_buf = pinned_alloc<csdr_complexf>(in_elems * 8), h_out_buf = pinned_alloc<csdr_complexf>((size_t)count * pitch * 8);
    const auto d_in_buf = ctx_alloc<csdr_complexf>(c, in_elems * 8 + 64), d_out_buf = ctx_alloc<csdr_complexf>(c, (size_t)count * pitch * 8 + 64);
    // batch header, rank 0 -> all: {blocks, end of stream, retunes, (channel, rate bits) x up to 16}
    enum { HDR_INTS = 3 + 2 * 16 };
    const auto h_hdr_buf = pinned_alloc<int>(HDR_INTS * sizeof(int), "pinned header");
    const auto d_hdr_buf = ctx_alloc<int>(c, HDR_INTS * sizeof(int) + 64);
    csdr_complexf *h_in = h_in_buf.get(), *h_out = h_out_buf.get(), *d_in = d_in_buf.get(), *d_out = d_out_buf.get();
    int *h_hdr = h_hdr_buf.get(), *d_hdr = d_hdr_buf.get();
    std::vector<int> counts(count);
    fprintf(stderr, "csdr fastddc_bank_cc: %d channels%s, fft_size = %d, input_size = %d, %d blocks per call\n", n_ch, multi ? " (sharded)" : "", ddc.fft_size, ddc.input_size, nb_max);
    if (multi) fprintf(stderr, "csdr fastddc_bank_cc: rank %d of %d serves channels %d .. %d\n", rank, world, first, first + count - 1);
    size_t have = 0;
    for (bool eof = false; !eof;) {
        int nb = 0, n_ret = 0; int ret_ch[16]; float ret_rate[16];
        if (rank == 0) {
            size_t got = 0;
            if (!read_full((char *)h_in + have * 8, (in_elems - have) * 8, &got)) eof = true;
            have += got / 8;
            if (ctl.fd) {
                // every complete line since the last poll is applied (several clients may retune between two blocks)
                ctl.lines.feed(ctl.fd);
                // at most 16 retunes travel in one batch header: further complete lines stay in the buffer for the next batch (none is dropped)
                while (n_ret < 16) {
                    const char *line = ctl.lines.next();
                    if (!line) break;
                    int ch = -1; float rate = 0;
                    if (sscanf(line, "%d %g", &ch, &rate) == 2 && ch >= 0 && ch < n_ch) { ret_ch[n_ret] = ch; ret_rate[n_ret] = rate; n_ret++; }
                }
            }
            nb = (int)(have / ddc.input_size);
        }
        if (multi) {
            if (rank == 0) {
                h_hdr[0] = nb; h_hdr[1] = eof ? 1 : 0; h_hdr[2] = n_ret;
                for (int i = 0; i < n_ret; i++) { h_hdr[3 + 2 * i] = ret_ch[i]; memcpy(&h_hdr[4 + 2 * i], &ret_rate[i], 4); }
                MUST(csdr_amd_h2d(c, d_hdr, h_hdr, HDR_INTS * sizeof(int)));
            }
            MUST(csdr_amd_comm_broadcast(comm, d_hdr, HDR_INTS * sizeof(int), 0));
            MUST(csdr_amd_d2h(c, h_hdr, d_hdr, HDR_INTS * sizeof(int)));
            nb = h_hdr[0]; eof = h_hdr[1] != 0; n_ret = h_hdr[2];
            for (int i = 0; i < n_ret; i++) { ret_ch[i] = h_hdr[3 + 2 * i]; memcpy(&ret_rate[i], &h_hdr[4 + 2 * i], 4); }
        }
        for (int i = 0; i < n_ret; i++) {
            MUST(csdr_amd_fastddc_bank_set_rate_global(bank, ret_ch[i], ret_rate[i]));      // every rank makes the call; a rank applies it to what it computes
            if (ret_ch[i] >= first && ret_ch[i] < first + count) fprintf(stderr, "csdr fastddc_bank_cc: channel %d retuned to %g\n", ret_ch[i], ret_rate[i]);
        }
        if (nb == 0) continue;
        const size_t used = (size_t)nb * ddc.input_size;
        if (rank == 0) MUST(csdr_amd_h2d(c, d_in, h_in, used * 8));
        MUST(csdr_amd_fastddc_bank_process(bank, d_in, nb, d_out, pitch, counts.data()));
        MUST(csdr_amd_d2h(c, h_out, d_out, (size_t)count * pitch * 8));
        for (int k = 0; k < count; k++) (void)write_fully(out_fd[first + k], h_out + (size_t)k * pitch, (size_t)counts[k] * 8);   // a failed write: this block is lost to that client, its descriptor stays
        if (rank == 0) { memmove(h_in, h_in + used, (have - used) * 8); have -= used; }
    }
    return 0;
}

// ------------------------------------------------------------------ the ddcd topology for FM clients: channelizer and NFM demodulators in one process
// Behind its `csdr fastddc_inv_cc` a ddcd / OpenWebRX client runs `fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff <audio_rate> | fastagc_ff | convert_f_s16`
// (README.md:87's tail).  Here: fastddc_bank_cc's loop with ONE csdr_amd_fmrx behind the bank; the N decimated channels stay in HBM and out_k receives s16 audio:
//   csdr fastddc_nfm_bank_s16 <decimation> <transition_bw> <window> <audio_rate> <ctl | -> <out_0> <shift_rate_0> [<out_1> <shift_rate_1> ...]
// out_k and ctl as in fastddc_bank_cc; a control line "<channel> <shift_rate>\n" retunes that channel from the next batch on, "<channel> reset\n" starts its
// demodulator, de-emphasis filter and AGC over (csdr_amd_fmrx_reset_channel).  The FM bank gives every channel the same number of samples per call; the
// channelizer's per-channel counts are equal by construction (its residual-shift bookkeeping does not depend on the rate), which is checked for every batch.
// One GPU only: with CSDR_AMD_WORLD set the command ends (fastddc_bank_cc is the one that shards a bank).
//   csdr fastddc_nfm_bank_s16 --squelch <block> <use_every_nth> <report_every_nth> <smeter_out> <decimation> ...      (the rest as above)
// puts squelch_and_smeter_cc (csdr.c:2192-2243) in front of every channel's demodulator, inside the bank object (csdr_amd_fmrx_create_squelched): blocks of <block>
// decimated samples, every level 0 (open) at the start; a control line "<channel> squelch <level>\n" sets that channel's level from the next block that starts.
// Every squelch block k with k mod (report_every_nth + 2) == report_every_nth + 1 writes one line "<channel> %g\n" per channel, its power, to <smeter_out>, which is
// written non-blocking as the reference writes its --outfifo: a line that does not fit is dropped.
// The same loop with ONE csdr_amd_wfmrx behind the bank, for broadcast FM clients (`fmdemod_quadri_cf | fractional_decimator_ff <frac_rate> | deemphasis_wfm_ff
// <audio_rate> <tau> | convert_f_s16`, the reference README's first receive line behind the channelizer):
//   csdr fastddc_wfm_bank_s16 <decimation> <transition_bw> <window> <frac_rate> <audio_rate> <tau> <ctl | -> <out_0> <shift_rate_0> [<out_1> <shift_rate_1> ...]
// with the same control lines; "<channel> reset\n" starts that channel's demodulator, held decimator input and de-emphasis over (csdr_amd_wfmrx_reset_channel).
//   csdr fastddc_wfm_bank_s16 --squelch <block> <use_every_nth> <report_every_nth> <smeter_out> <decimation> ...      (the rest as above)
// is the NFM command's --squelch on csdr_amd_wfmrx_create_squelched: the same control line, the same report lines.
int run_fm_bank(csdr_amd_ctx *c, int argc, char **argv, size_t block, bool wfm)
{
    int sqB = 0, sq_d = 1, sq_report = 0; const char *smeter_path = nullptr;
    if (argc > 2 && !strcmp(argv[2], "--squelch")) {
        if (argc < 7 || sscanf(argv[3], "%d", &sqB) != 1 || sscanf(argv[4], "%d", &sq_d) != 1 || sscanf(argv[5], "%d", &sq_report) != 1)
            return badsyntax(wfm ? "usage: fastddc_wfm_bank_s16 --squelch <block> <use_every_nth> <report_every_nth> <smeter_out> <decimation> ..."
                                 : "usage: fastddc_nfm_bank_s16 --squelch <block> <use_every_nth> <report_every_nth> <smeter_out> <decimation> ...");
        if (sqB < 1) return badsyntax("the squelch block must be >= 1");
        if (sq_d <= 0) return badsyntax("use_every_nth <= 0 is invalid");
        if (sq_report <= 0) return badsyntax("report_every_nth <= 0 is invalid");
        smeter_path = argv[6];
        argv += 5; argc -= 5;                                          // argv[2] is <decimation> again
    }
    const int a0 = wfm ? 8 : 6;                                        // argv index of the control channel; the <out_k> <rate_k> pairs follow it
    if (argc < a0 + 3 || (argc - a0 - 1) % 2)
        return badsyntax(wfm ? "usage: fastddc_wfm_bank_s16 <decimation> <transition_bw> <window> <frac_rate> <audio_rate> <tau> <ctl|-> <out_0> <rate_0> [<out_k> <rate_k> ...]"
                             : "usage: fastddc_nfm_bank_s16 <decimation> <transition_bw> <window> <audio_rate> <ctl|-> <out_0> <rate_0> [<out_k> <rate_k> ...]");
    if (getenv("CSDR_AMD_WORLD")) return badsyntax("runs on one GPU only: CSDR_AMD_WORLD is set (fastddc_bank_cc is the command that shards a bank over several)");
    int D = 0, audio_rate = 0; float tbw = 0.05f, frac_rate = 0, tau = 0; sscanf(argv[2], "%d", &D); sscanf(argv[3], "%g", &tbw); sscanf(argv[wfm ? 6 : 5], "%d", &audio_rate);
    if (wfm && (sscanf(argv[5], "%g", &frac_rate) != 1 || sscanf(argv[7], "%g", &tau) != 1)) return badsyntax("frac_rate and tau must be numbers");
    const int window = window_from(argv[4]);
    const int n_ch = (argc - a0 - 1) / 2;
    Fds ctl_fd(1, -1); LineSplitter lines;
    if (strcmp(argv[a0], "-")) {
        ctl_fd[0] = open_spec(argv[a0], O_RDONLY | O_NONBLOCK);
        if (ctl_fd[0] < 0) return badsyntax("cannot open the control channel");
        fcntl(ctl_fd[0], F_SETFL, fcntl(ctl_fd[0], F_GETFL, 0) | O_NONBLOCK);
    }
    std::vector<float> rates(n_ch);
    for (int k = 0; k < n_ch; k++) if (sscanf(argv[a0 + 2 + 2 * k], "%g", &rates[k]) != 1) return badsyntax("every rate must be a number");
    csdr_fastddc_t ddc;
    if (csdr_amd_fastddc_init(&ddc, tbw, D, 0)) return badsyntax("error in fastddc_init()");
    int nb_max = (int)(block / ddc.input_size); if (nb_max < 1) nb_max = 1;
    Owned<csdr_amd_fastddc_bank, csdr_amd_fastddc_bank_destroy> bank(csdr_amd_fastddc_bank_create(c, tbw, D, rates.data(), n_ch, window, nb_max));
    if (!bank) die("fastddc_bank create");
    const size_t pitch = ((size_t)csdr_amd_fastddc_bank_max_output(bank.get(), nb_max) + 9) & ~(size_t)1;      // even: the FM bank's one-kernel path reads two samples a lane
    Owned<csdr_amd_fmrx, csdr_amd_fmrx_destroy> fm; Owned<csdr_amd_wfmrx, csdr_amd_wfmrx_destroy> wf;
    if (wfm && sqB) wf.reset(csdr_amd_wfmrx_create_squelched(c, n_ch, frac_rate, 12, nullptr, 0, 1024, tau, audio_rate, pitch, sqB, sq_d, nullptr));
    else if (wfm) wf.reset(csdr_amd_wfmrx_create(c, n_ch, frac_rate, 12, nullptr, 0, 1024, tau, audio_rate, pitch));     // fractional_decimator_ff's defaults (csdr.c:1470-1472)
    else if (sqB) fm.reset(csdr_amd_fmrx_create_squelched(c, n_ch, audio_rate, 1024, 1.0f, 1.0f, pitch, sqB, sq_d, nullptr));
    else fm.reset(csdr_amd_fmrx_create(c, n_ch, audio_rate, 1024, 1.0f, 1.0f, pitch));      // limit_ff and fastagc_ff defaults (csdr.c:673-686, 1379-1391)
    if (!fm && !wf) return badsyntax(csdr_amd_last_error());
    Fds smeter_fd(1, -1);
    const size_t p_pitch = sqB ? pitch / (size_t)sqB + 1 : 0;           // the most squelch blocks of a call
    CtxBuf<float> d_power; std::vector<float> h_power;
    if (sqB) {
        smeter_fd[0] = open_spec(smeter_path, O_WRONLY | O_CREAT | O_TRUNC);
        if (smeter_fd[0] < 0) return badsyntax("cannot open the S-meter output");
        fcntl(smeter_fd[0], F_SETFL, fcntl(smeter_fd[0], F_GETFL, 0) | O_NONBLOCK);
        d_power = ctx_alloc<float>(c, (size_t)n_ch * p_pitch * 4 + 64); h_power.resize((size_t)n_ch * p_pitch);
    }
    const size_t a_pitch = ((size_t)(wfm ? csdr_amd_wfmrx_max_output(wf.get(), (long long)pitch) : csdr_amd_fmrx_max_output(fm.get(), (long long)pitch)) + 15) & ~(size_t)7;
    Fds out_fd(n_ch, -1);
    for (int k = 0; k < n_ch; k++) {
        out_fd[k] = open_spec(argv[a0 + 1 + 2 * k], O_WRONLY | O_CREAT | O_TRUNC);
        if (out_fd[k] < 0) { fprintf(stderr, "csdr %s: cannot open output %s\n", g_cmd, argv[a0 + 1 + 2 * k]); return -1; }
    }
    const size_t in_elems = (size_t)nb_max * ddc.input_size;
    const auto h_in = pinned_alloc<csdr_complexf>(in_elems * 8);
    const auto h_out = pinned_alloc<int16_t>((size_t)n_ch * a_pitch * 2);
    const auto d_in = ctx_alloc<csdr_complexf>(c, in_elems * 8 + 64), d_bb = ctx_alloc<csdr_complexf>(c, (size_t)n_ch * pitch * 8 + 64);
    const auto d_out = ctx_alloc<int16_t>(c, (size_t)n_ch * a_pitch * 2 + 64);
    std::vector<int> counts(n_ch);
    fprintf(stderr, "csdr %s: %d channels, fft_size = %d, input_size = %d, %d blocks per call, audio rate %d\n", g_cmd, n_ch, ddc.fft_size, ddc.input_size, nb_max, audio_rate);
    size_t have = 0;
    for (bool eof = false; !eof;) {
        size_t got = 0;
        if (!read_full((char *)h_in.get() + have * 8, (in_elems - have) * 8, &got)) eof = true;
        have += got / 8;
        if (ctl_fd[0] >= 0)
            while (lines.feed(ctl_fd[0])) while (const char *line = lines.next()) {
                int ch = -1; char what[32] = "";
                if (sscanf(line, "%d %31s", &ch, what) != 2 || ch < 0 || ch >= n_ch) continue;
                float rate = 0, level = 0;
                if (sqB && !strcmp(what, "squelch")) {
                    if (sscanf(line, "%d squelch %g", &ch, &level) != 2) continue;
                    MUST(wfm ? csdr_amd_wfmrx_set_squelch_level(wf.get(), ch, level) : csdr_amd_fmrx_set_squelch_level(fm.get(), ch, level));
                    fprintf(stderr, "csdr %s: channel %d squelch level is %g\n", g_cmd, ch, level);
                } else if (!strcmp(what, "reset")) {
                    MUST(wfm ? csdr_amd_wfmrx_reset_channel(wf.get(), ch) : csdr_amd_fmrx_reset_channel(fm.get(), ch));
                    fprintf(stderr, "csdr %s: channel %d reset\n", g_cmd, ch);
                } else if (sscanf(what, "%g", &rate) == 1) {
                    MUST(csdr_amd_fastddc_bank_set_rate(bank.get(), ch, rate));
                    fprintf(stderr, "csdr %s: channel %d retuned to %g\n", g_cmd, ch, rate);
                }
            }
        const int nb = (int)(have / ddc.input_size);
        if (nb == 0) continue;
        const size_t used = (size_t)nb * ddc.input_size;
        MUST(csdr_amd_h2d(c, d_in.get(), h_in.get(), used * 8));
        MUST(csdr_amd_fastddc_bank_process(bank.get(), d_in.get(), nb, d_bb.get(), pitch, counts.data()));
        for (int k = 1; k < n_ch; k++)
            if (counts[k] != counts[0]) { fprintf(stderr, "csdr %s: the channelizer wrote %d samples for channel %d and %d for channel 0: the FM bank advances its channels in lockstep\n", g_cmd, counts[k], k, counts[0]); return -1; }
        const long long sq_k0 = !sqB ? 0 : wfm ? csdr_amd_wfmrx_squelch_block_index(wf.get()) : csdr_amd_fmrx_squelch_block_index(fm.get());
        int sq_nb = 0;
        const long long na = wfm && sqB ? csdr_amd_wfmrx_process_squelched(wf.get(), d_bb.get(), pitch, counts[0], d_out.get(), nullptr, a_pitch, d_power.get(), p_pitch, nullptr, &sq_nb)
                           : wfm ? csdr_amd_wfmrx_process(wf.get(), d_bb.get(), pitch, counts[0], d_out.get(), nullptr, a_pitch)
                           : sqB ? csdr_amd_fmrx_process_squelched(fm.get(), d_bb.get(), pitch, counts[0], d_out.get(), nullptr, a_pitch, d_power.get(), p_pitch, nullptr, &sq_nb)
                                 : csdr_amd_fmrx_process(fm.get(), d_bb.get(), pitch, counts[0], d_out.get(), nullptr, a_pitch);
        MUST(na);
        bool sq_due = false;
        for (int k = 0; k < sq_nb && !sq_due; k++) sq_due = csdr_amd_squelch_report_due(sq_report, sq_k0 + k) != 0;
        if (sq_due) {
            MUST(csdr_amd_d2h(c, h_power.data(), d_power.get(), (size_t)n_ch * p_pitch * 4));
            for (int k = 0; k < sq_nb; k++) if (csdr_amd_squelch_report_due(sq_report, sq_k0 + k))
                for (int ch = 0; ch < n_ch; ch++) {
                    char line[128]; const int len = snprintf(line, sizeof line, "%d %g\n", ch, h_power[(size_t)ch * p_pitch + k]);
                    (void)!write(smeter_fd[0], line, (size_t)len);       // non-blocking: a line that does not fit is dropped (csdr.c:2211-2228)
                }
        }
        if (na > 0) {
            MUST(csdr_amd_d2h(c, h_out.get(), d_out.get(), (size_t)n_ch * a_pitch * 2));
            for (int k = 0; k < n_ch; k++)
                if (out_fd[k] >= 0 && !write_fully(out_fd[k], h_out.get() + (size_t)k * a_pitch, (size_t)na * 2)) { close(out_fd[k]); out_fd[k] = -1; }
        }
        memmove(h_in.get(), h_in.get() + used, (have - used) * 8); have -= used;
    }
    return 0;
}

// ------------------------------------------------------------------ one shifter per client on one wideband stream (csdr.c:881-923, ddcd_old.h:51-61) in one process
//   csdr shift_bank_cc <addition|math|table[:size]> <ctl | -> <out_0> <rate_0> [<out_1> <rate_1> ...]
// reads ONE complexf stream from stdin and writes N shifted streams through one csdr_amd_shiftbank (the input row shared by all streams).  out_k and ctl as in
// fastddc_bank_cc; a control line "<channel> <rate>\n" retunes that channel from the next block on, as `shift_addition_cc --fifo` does between two reads.
// Blocks are CSDR_AMD_BANK_BLOCK samples (default 262144, a multiple of 1024); out_k carries what `csdr shift_<variant>_cc <rate_k>` writes for the same input.
size_t bank_block();
int run_shift_bank(csdr_amd_ctx *c, int argc, char **argv)
{
    if (argc < 6 || (argc - 4) % 2) return badsyntax("usage: shift_bank_cc <addition|math|table[:size]> <ctl|-> <out_0> <rate_0> [<out_k> <rate_k> ...]");
    int variant = -1, aux = 0;
    if (!strcmp(argv[2], "addition")) variant = CSDR_SHIFT_ADDITION;
    else if (!strcmp(argv[2], "math")) variant = CSDR_SHIFT_MATH;
    else if (!strncmp(argv[2], "table", 5) && (!argv[2][5] || argv[2][5] == ':')) { variant = CSDR_SHIFT_TABLE; aux = 65536; if (argv[2][5]) sscanf(argv[2] + 6, "%d", &aux); }   // csdr.c:731
    if (variant < 0 || aux < 0) return badsyntax("the variant is addition, math or table[:size]");
    const int n_ch = (argc - 4) / 2;
    Fds ctl_fd(1, -1); LineSplitter lines;
    if (strcmp(argv[3], "-")) {
        ctl_fd[0] = open_spec(argv[3], O_RDONLY | O_NONBLOCK);
        if (ctl_fd[0] < 0) return badsyntax("cannot open the control channel");
        fcntl(ctl_fd[0], F_SETFL, fcntl(ctl_fd[0], F_GETFL, 0) | O_NONBLOCK);
    }
    std::vector<float> rates(n_ch);
    for (int k = 0; k < n_ch; k++) if (sscanf(argv[5 + 2 * k], "%g", &rates[k]) != 1) return badsyntax("every rate must be a number");
    const size_t T = bank_block() / 1024 * 1024;
    Owned<csdr_amd_shiftbank, csdr_amd_shiftbank_destroy> bank(csdr_amd_shiftbank_create(c, variant, n_ch, rates.data(), 1024, aux, CSDR_AMD_SHIFTBANK_IN_CF32, T));
    if (!bank) die("shiftbank create");
    Fds out_fd(n_ch, -1);
    for (int k = 0; k < n_ch; k++) {
        out_fd[k] = open_spec(argv[4 + 2 * k], O_WRONLY | O_CREAT | O_TRUNC);
        if (out_fd[k] < 0) { fprintf(stderr, "csdr %s: cannot open output %s\n", g_cmd, argv[4 + 2 * k]); return -1; }
    }
    const auto h_in = pinned_alloc<csdr_complexf>(T * 8), h_out = pinned_alloc<csdr_complexf>((size_t)n_ch * T * 8);
    const auto d_in = ctx_alloc<csdr_complexf>(c, T * 8 + 64), d_out = ctx_alloc<csdr_complexf>(c, (size_t)n_ch * T * 8 + 64);
    fprintf(stderr, "csdr %s: %d channels, %zu samples per block\n", g_cmd, n_ch, T);
    for (bool eof = false; !eof;) {
        size_t got = 0;
        if (!read_full(h_in.get(), T * 8, &got)) eof = true;
        const size_t n = got / 8;
        if (ctl_fd[0] >= 0)
            while (lines.feed(ctl_fd[0])) while (const char *line = lines.next()) {
                int ch = -1; float rate = 0;
                if (sscanf(line, "%d %g", &ch, &rate) != 2 || ch < 0 || ch >= n_ch) continue;
                MUST(csdr_amd_shiftbank_set_rate(bank.get(), ch, rate));
                fprintf(stderr, "csdr %s: channel %d reinitialized to %g\n", g_cmd, ch, rate);
            }
        if (!n) continue;
        MUST(csdr_amd_h2d(c, d_in.get(), h_in.get(), n * 8));
        MUST(csdr_amd_shiftbank_process(bank.get(), d_in.get(), 0, d_out.get(), T, n));
        MUST(csdr_amd_d2h(c, h_out.get(), d_out.get(), (size_t)n_ch * T * 8));
        for (int k = 0; k < n_ch; k++)
            if (out_fd[k] >= 0 && !write_fully(out_fd[k], h_out.get() + (size_t)k * T, n * 8)) { close(out_fd[k]); out_fd[k] = -1; }
    }
    return 0;
}

// ------------------------------------------------------------------ f4, first half: N-stream host ingest into the batch API
// nmux / ddcd fan one source out to N clients, each client = one `csdr ... | csdr ...` pipeline of processes (nmux.cpp:177-283, ddcd_old.cpp:474-492).
// The device batch API wants the opposite shape: N streams side by side in ONE call.  These commands are that producer:
//   csdr wfm_bank_u8_s16 <shift_rate> <in_0> <out_0> [<in_1> <out_1> ...]      N u8 IQ streams -> N s16 audio streams through ONE fused WFM chain object
//   csdr nfm_bank_u8_s16 <shift_rate> <in_0> <out_0> [<in_1> <out_1> ...]      the same through the NFM chain object (README.md:87 defaults)
//   csdr am_bank_u8_s16  <shift_rate> <in_0> <out_0> [<in_1> <out_1> ...]      the same through the AM chain object (README.md:95 defaults: decimation 50, tbw 0.005)
//   csdr ssb_bank_u8_s16 [--lsb] <shift_rate> <in_0> <out_0> [...]             the same through the SSB chain object (README.md:110 defaults: passband 0 0.1 0.05;
//                                                                              --lsb: -0.1 0)
//   csdr ssb_bank_u8_s16 --passbands lo:hi[,lo:hi,...] <shift_rate> ...        one passband for all streams or one per stream (transition bandwidth 0.05 for all);
//                                                                              not together with --lsb
// in_k / out_k: a path (file or fifo) or fd:<n>.  Every pass reads one block of CSDR_AMD_BANK_BLOCK samples (default 262144, a multiple of 1024) from
// EVERY input (the streams advance in lockstep, like the clients of one nmux), uploads them as the rows of one batch, runs the chain once and writes
// each row's audio to its output.  The pass in which the first stream ends is the last one (lockstep streams end together).
//   <shift_rate> may be a comma-separated list, one rate per stream (ddcd tunes every client on its own: ddcd_old.h:51-61);
//   --ctl <fifo | fd:<n>> in front of it: control lines "<stream> <rate>\n", applied between two passes exactly as `shift_addition_cc --fifo` applies a new rate
//   between two reads (csdr.c:881-923: the phase carries over).  ssb_bank_u8_s16 also takes "<stream> bp <low> <high>\n": that stream's passband, as a retuned
//   `bandpass_fir_fft_cc --fifo` (csdr.c:1817-1881), from the first sample the bank's filter has not consumed yet.
//   csdr am_bank_u8_s16 --squelch <use_every_nth> <report_every_nth> <smeter_out> ...   and the same for ssb_bank_u8_s16 (the rest as above, --lsb, --passbands and
//   --ctl included): squelch_and_smeter_cc (csdr.c:2192-2243) between every stream's channel filter and its demodulator, inside the bank object
//   (csdr_amd_amssb_enable_squelch): blocks of the chain's 1024 decimated samples, every level 0 (open) at the start; a control line "<stream> squelch <level>\n"
//   sets that stream's level from the next block that starts.  Every block k with k mod (report_every_nth + 2) == report_every_nth + 1 writes one line
//   "<stream> %g\n" per stream, its power, to <smeter_out>, non-blocking as the reference writes its --outfifo: a line that does not fit is dropped.
size_t bank_block() { size_t T = 262144; if (const char *e = getenv("CSDR_AMD_BANK_BLOCK")) { long v = atol(e); if (v >= 1024) T = (size_t)v; } return T; }

// The lockstep loop of the stream banks.  specs: in_0 out_0 in_1 out_1 ... (S pairs).  Every pass reads T samples of u8 IQ from EVERY input into the rows of one batch
// (in_pitch bytes apart; what an input could not fill is 0x80, the u8 zero), uploads it and lets `process` run the bank's object once over the samples that ALL inputs gave:
// (d_in, d_out, samples) -> bytes to write per row (rows out_pitch bytes apart in d_out), 0 for none.  `between`, if any, runs in front of every process (the --ctl retunes).
// The pass in which the first input ends is the last one, and an input that ends with nothing left ends the process without another pass.  An output that cannot be
// written to is closed; the others carry on.
int run_lockstep(csdr_amd_ctx *c, char **specs, int S, size_t T, size_t in_pitch, size_t out_pitch,
                 const std::function<size_t(const uint8_t *, uint8_t *, size_t)> &process, const std::function<void()> &between = nullptr)
{
    Fds in_fd(S, -1), out_fd(S, -1);
    for (int k = 0; k < S; k++) {
        in_fd[k] = open_spec(specs[2 * k], O_RDONLY); out_fd[k] = open_spec(specs[2 * k + 1], O_WRONLY | O_CREAT | O_TRUNC);
        if (in_fd[k] < 0 || out_fd[k] < 0) { fprintf(stderr, "csdr %s: cannot open %s / %s\n", g_cmd, specs[2 * k], specs[2 * k + 1]); return -1; }
    }
    const auto h_in = pinned_alloc<uint8_t>((size_t)S * in_pitch), h_out = pinned_alloc<uint8_t>((size_t)S * out_pitch);
    const auto d_in = ctx_alloc<uint8_t>(c, (size_t)S * in_pitch + 256), d_out = ctx_alloc<uint8_t>(c, (size_t)S * out_pitch + 256);
    fprintf(stderr, "csdr %s: %d streams, %zu samples per stream and pass\n", g_cmd, S, T);
    for (size_t got_min = T; got_min == T;) {
        for (int k = 0; k < S; k++) {
            uint8_t *row = h_in.get() + (size_t)k * in_pitch;
            const size_t have = read_fully(in_fd[k], row, in_pitch);
            memset(row + have, 0x80, in_pitch - have);
            if (have / 2 < got_min) got_min = have / 2;
        }
        if (!got_min) break;
        if (between) between();
        MUST(csdr_amd_h2d(c, d_in.get(), h_in.get(), (size_t)S * in_pitch));
        const size_t bytes = process(d_in.get(), d_out.get(), got_min);
        if (!bytes) continue;
        MUST(csdr_amd_d2h(c, h_out.get(), d_out.get(), (size_t)S * out_pitch));
        for (int k = 0; k < S; k++)
            if (out_fd[k] >= 0 && !write_fully(out_fd[k], h_out.get() + (size_t)k * out_pitch, bytes)) { close(out_fd[k]); out_fd[k] = -1; }
    }
    return 0;
}

enum { BANK_WFM, BANK_NFM, BANK_AM, BANK_SSB };
int run_stream_bank(csdr_amd_ctx *c, int argc, char **argv, int kind)
{
    const bool nfm = kind == BANK_NFM, amssb = kind == BANK_AM || kind == BANK_SSB;
    bool lsb = false, sq = false;
    int sq_d = 1, sq_report = 0; const char *smeter_path = nullptr;
    if (amssb && argc > 2 && !strcmp(argv[2], "--squelch")) {
        if (argc < 6 || sscanf(argv[3], "%d", &sq_d) != 1 || sscanf(argv[4], "%d", &sq_report) != 1)
            return badsyntax("usage: --squelch <use_every_nth> <report_every_nth> <smeter_out> [--lsb | --passbands ...] [--ctl <fifo|fd:n>] <shift_rate[,...]> <in_0> <out_0> ...");
        if (sq_d <= 0) return badsyntax("use_every_nth <= 0 is invalid");
        if (sq_report <= 0) return badsyntax("report_every_nth <= 0 is invalid");
        smeter_path = argv[5]; sq = true;
        argv += 4; argc -= 4;
    }
    if (kind == BANK_SSB && argc > 2 && !strcmp(argv[2], "--lsb")) { lsb = true; argv += 1; argc -= 1; }
    std::vector<float> bands;                                          // --passbands: low_0, high_0, low_1, ...
    if (kind == BANK_SSB && argc > 2 && !strcmp(argv[2], "--passbands")) {
        if (lsb) return badsyntax("--lsb and --passbands exclude each other");
        if (argc < 4) return badsyntax("--passbands needs lo:hi[,lo:hi,...]");
        for (const char *q = argv[3]; ;) {
            char *e1 = nullptr, *e2 = nullptr;
            const float lo = strtof(q, &e1);
            if (e1 == q || *e1 != ':') return badsyntax("--passbands: every passband is lo:hi");
            const float hi = strtof(e1 + 1, &e2);
            if (e2 == e1 + 1 || (*e2 && *e2 != ',') || !(lo < hi)) return badsyntax("--passbands: every passband is lo:hi with lo < hi");
            bands.push_back(lo); bands.push_back(hi);
            if (!*e2) break;
            q = e2 + 1;
        }
        argv += 2; argc -= 2;
        if (argc > 2 && !strcmp(argv[2], "--lsb")) return badsyntax("--lsb and --passbands exclude each other");
    }
    Fds ctl_fd(1, -1);
    if (argc > 3 && !strcmp(argv[2], "--ctl")) {
        ctl_fd[0] = open_spec(argv[3], O_RDONLY | O_NONBLOCK);
        if (ctl_fd[0] < 0) { fprintf(stderr, "csdr %s: cannot open the control channel %s\n", g_cmd, argv[3]); return -1; }
        fcntl(ctl_fd[0], F_SETFL, fcntl(ctl_fd[0], F_GETFL, 0) | O_NONBLOCK);
        argv += 2; argc -= 2;
    }
    if (argc < 5 || (argc - 3) % 2) return badsyntax("usage: [--ctl <fifo|fd:n>] <shift_rate[,rate_1,...]> <in_0> <out_0> [<in_k> <out_k> ...]   (paths, fifos or fd:<n>)");
    const int S = (argc - 3) / 2;
    std::vector<float> rates;
    for (const char *q = argv[2]; *q;) { char *end = nullptr; const float v = strtof(q, &end); if (end == q) return badsyntax("shift_rate must be a number or a comma-separated list"); rates.push_back(v); q = *end == ',' ? end + 1 : end; if (*end && *end != ',') return badsyntax("shift_rate must be a number or a comma-separated list"); }
    if (rates.size() != 1 && (int)rates.size() != S) return badsyntax("as many shift rates as streams (or one for all)");
    if (bands.size() > 2 && (int)bands.size() != 2 * S) return badsyntax("as many passbands as streams (or one for all)");
    // (fewer than 16 streams: the rate-per-stream object also when they share one rate -- its kernel fills all 16 columns of a tile with time segments of ONE stream,
    // the shared-rate kernel needs 16 streams to fill them)
    const bool per_stream = rates.size() > 1 || ctl_fd[0] >= 0 || (S < 16 && !getenv("CSDR_AMD_CLI_SHARED"));
    if (per_stream && rates.size() == 1) rates.assign(S, rates[0]);
    const float shift = rates[0];
    const size_t T = bank_block() / 1024 * 1024;
    const int D = kind == BANK_WFM ? 10 : 50; const float tbw = kind == BANK_WFM ? 0.05f : 0.005f;
    const int nt = csdr_amd_firdes_filter_len(tbw);
    std::vector<float> taps(nt); csdr_amd_firdes_lowpass_f(taps.data(), nt, 0.5f / (float)D, CSDR_WINDOW_HAMMING);
    Owned<csdr_amd_wfm, csdr_amd_wfm_destroy> w; Owned<csdr_amd_nfm, csdr_amd_nfm_destroy> n; Owned<csdr_amd_amssb, csdr_amd_amssb_destroy> a;
    if (amssb) {
        csdr_amd_amssb_params ap;
        MUST(csdr_amd_amssb_params_default(&ap, kind == BANK_AM ? CSDR_AMD_AMSSB_AM : CSDR_AMD_AMSSB_SSB));
        std::vector<csdr_complexf> bp; int fft = 0;
        if (kind == BANK_SSB) {                                       // bandpass_fir_fft_cc 0 0.1 0.05 (the transform's size as csdr.c:1834-1836 chooses it)
            const int bl = csdr_amd_firdes_filter_len(0.05f);
            const float lo = !bands.empty() ? bands[0] : lsb ? -0.1f : 0.f, hi = !bands.empty() ? bands[1] : lsb ? 0.f : 0.1f;
            bp.resize(bl); csdr_amd_firdes_bandpass_c(bp.data(), bl, lo, hi, CSDR_WINDOW_HAMMING);
            fft = csdr_amd_next_pow2(bl); if (fft - bl < 200) fft *= 2;
        }
        a.reset(per_stream ? csdr_amd_amssb_create_rates(c, &ap, S, rates.data(), D, taps.data(), nt, bp.data(), (int)bp.size(), fft, T)
                           : csdr_amd_amssb_create(c, &ap, S, shift, D, taps.data(), nt, bp.data(), (int)bp.size(), fft, T));
    }
    else if (nfm && per_stream) n.reset(csdr_amd_nfm_create_rates(c, S, rates.data(), D, taps.data(), nt, 48000, 1024, 1.0f, 1.0f, T));
    else if (nfm) n.reset(csdr_amd_nfm_create(c, S, shift, D, taps.data(), nt, 48000, 1024, 1.0f, 1.0f, T));
    else if (per_stream) w.reset(csdr_amd_wfm_create_rates(c, S, rates.data(), D, taps.data(), nt, 5, 50e-6f, 48000, T));
    else w.reset(csdr_amd_wfm_create(c, S, shift, D, taps.data(), nt, 5, 50e-6f, 48000, T));
    if (!w && !n && !a) die("bank create");
    if (bands.size() > 2) for (int k = 0; k < S; k++) MUST(csdr_amd_amssb_set_passband(a.get(), k, bands[2 * k], bands[2 * k + 1], CSDR_WINDOW_HAMMING));
    const size_t in_pitch = 2 * T, out_pitch = ((T / 50 + 4096 + 63) / 64) * 64;      // out_pitch: s16 samples
    Fds smeter_fd(1, -1);
    size_t p_pitch = 0; CtxBuf<float> d_power; std::vector<float> h_power;
    if (sq) {
        MUST(csdr_amd_amssb_enable_squelch(a.get(), sq_d, nullptr));
        smeter_fd[0] = open_spec(smeter_path, O_WRONLY | O_CREAT | O_TRUNC);
        if (smeter_fd[0] < 0) return badsyntax("cannot open the S-meter output");
        fcntl(smeter_fd[0], F_SETFL, fcntl(smeter_fd[0], F_GETFL, 0) | O_NONBLOCK);
        p_pitch = (size_t)csdr_amd_amssb_max_out(a.get(), (long long)T) / 1024 + 1;     // the most blocks of a pass (the chain's block is 1024)
        d_power = ctx_alloc<float>(c, (size_t)S * p_pitch * 4 + 64); h_power.resize((size_t)S * p_pitch);
    }
    // a short final block: whole 1024-sample chunks of the shortest stream (the chain objects take a ragged LAST block only)
    auto pass = [&](const uint8_t *d_in, uint8_t *d_out, size_t nproc) {
        if (sq) {
            const long long k0 = csdr_amd_amssb_squelch_block_index(a.get());
            int nb = 0;
            const long long na = csdr_amd_amssb_process_squelched(a.get(), d_in, in_pitch, (long long)nproc, (int16_t *)d_out, nullptr, out_pitch, d_power.get(), p_pitch, nullptr, &nb);
            MUST(na);
            bool due = false;
            for (int k = 0; k < nb && !due; k++) due = csdr_amd_squelch_report_due(sq_report, k0 + k) != 0;
            if (due) {
                MUST(csdr_amd_d2h(c, h_power.data(), d_power.get(), (size_t)S * p_pitch * 4));
                for (int k = 0; k < nb; k++) if (csdr_amd_squelch_report_due(sq_report, k0 + k))
                    for (int ch = 0; ch < S; ch++) {
                        char line[128]; const int len = snprintf(line, sizeof line, "%d %g\n", ch, h_power[(size_t)ch * p_pitch + k]);
                        (void)!write(smeter_fd[0], line, (size_t)len);       // non-blocking: a line that does not fit is dropped (csdr.c:2211-2228)
                    }
            }
            return (size_t)na * 2;
        }
        const long na = amssb ? (long)csdr_amd_amssb_process(a.get(), d_in, in_pitch, (long long)nproc, (int16_t *)d_out, nullptr, out_pitch) :
                        nfm ? csdr_amd_nfm_process(n.get(), d_in, in_pitch, nproc, (int16_t *)d_out, nullptr, out_pitch) : csdr_amd_wfm_process(w.get(), d_in, in_pitch, nproc, (int16_t *)d_out, nullptr, out_pitch);
        MUST(na);
        return (size_t)na * 2;
    };
    // retunes that have arrived: complete lines only, the rest waits for the next pass
    LineSplitter lines;
    auto retunes = [&]() {
        while (lines.feed(ctl_fd[0])) while (const char *line = lines.next()) {
            int st = -1; float rv = 0, lo = 0, hi = 0;
            if (kind == BANK_SSB && sscanf(line, "%d bp %g %g", &st, &lo, &hi) == 3) {
                if (st < 0 || st >= S || !(lo < hi)) continue;
                MUST(csdr_amd_amssb_set_passband(a.get(), st, lo, hi, CSDR_WINDOW_HAMMING));
                fprintf(stderr, "csdr %s: stream %d passband reinitialized to %g %g\n", g_cmd, st, lo, hi);
                continue;
            }
            if (sq && sscanf(line, "%d squelch %g", &st, &rv) == 2) {
                if (st < 0 || st >= S) continue;
                MUST(csdr_amd_amssb_set_squelch_level(a.get(), st, rv));
                fprintf(stderr, "csdr %s: stream %d squelch level is %g\n", g_cmd, st, rv);
                continue;
            }
            if (sscanf(line, "%d %g", &st, &rv) != 2 || st < 0 || st >= S) continue;
            MUST(amssb ? csdr_amd_amssb_set_rate(a.get(), st, rv) : nfm ? csdr_amd_nfm_set_rate(n.get(), st, rv) : csdr_amd_wfm_set_rate(w.get(), st, rv));
            fprintf(stderr, "csdr %s: stream %d reinitialized to %g\n", g_cmd, st, rv);
        }
    };
    return run_lockstep(c, argv + 3, S, T, in_pitch, 2 * out_pitch, pass, ctl_fd[0] >= 0 ? std::function<void()>(retunes) : nullptr);
}

// csdr waterfall_bank_u8 <fft> <every_n> <window> <add_db> <avg> <db|adpcm> <in_0> <out_0> [<in_1> <out_1> ...]: N u8 IQ streams through ONE waterfall object
// (the batch API from the command line).  Lockstep like wfm_bank_u8_s16: every pass reads CSDR_AMD_BANK_BLOCK samples (default 262144) from every input; the
// pass in which the first stream ends is the last one.  Each output gets the rows of its stream, byte-identical to `csdr waterfall_u8` on that input alone.
int run_waterfall_bank(csdr_amd_ctx *c, int argc, char **argv)
{
    if (argc < 10 || (argc - 8) % 2) return badsyntax("usage: <fft_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm> <in_0> <out_0> [<in_k> <out_k> ...]   (paths, fifos or fd:<n>)");
    int fft = 0, every = 0, avg = 0; float add_db = 0;
    sscanf(argv[2], "%d", &fft); sscanf(argv[3], "%d", &every); sscanf(argv[5], "%g", &add_db); sscanf(argv[6], "%d", &avg);
    if (csdr_amd_log2n(fft) < 1 || every <= 0 || avg <= 0) return badsyntax("fft_size must be a power of two >= 2, every_n and avgnumber positive");
    const bool adpcm = !strcmp(argv[7], "adpcm");
    const int S = (argc - 8) / 2;
    const size_t T = bank_block();
    Owned<csdr_amd_waterfall, csdr_amd_waterfall_destroy> w(csdr_amd_waterfall_create(c, fft, every, window_from(argv[4]), avg, add_db, CSDR_AMD_WF_IN_U8, adpcm ? CSDR_AMD_WF_OUT_ADPCM : CSDR_AMD_WF_OUT_DB, S, T));
    if (!w) die("waterfall_create");
    const size_t row_bytes = adpcm ? (size_t)(fft + 10) / 2 : 4 * (size_t)fft;
    const size_t out_pitch = ((T + fft) / every / avg + 2) * row_bytes;
    auto pass = [&](const uint8_t *d_in, uint8_t *d_out, size_t n) {
        int rows = 0;
        MUST(csdr_amd_waterfall_process(w.get(), d_in, n, T, d_out, out_pitch, &rows));
        return rows > 0 ? (size_t)rows * row_bytes : (size_t)0;
    };
    return run_lockstep(c, argv + 8, S, T, 2 * T, out_pitch, pass);
}
