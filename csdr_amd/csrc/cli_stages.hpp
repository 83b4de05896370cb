// cli_stages.hpp -- included by csdr_cli.cpp inside its anonymous namespace: the streaming operators and make_stage(), which builds one from a command line
// One streaming operator: consumes in_elem-byte elements, produces out_elem-byte elements.
struct Stage {
    size_t in_elem = 4, out_elem = 4;
    size_t min_block = 0;          // run() uses blocks of at least 4x this many elements (operators with a long history)
    size_t granule = 1;            // process() is only called with n_in a multiple of this (except at EOF when flush_partial)
    bool flush_partial = true;     // at EOF, a final n_in % granule != 0 call is allowed
    size_t max_block = 0;          // as the first operator of a run: at most this many elements per pass (0: no limit); for operators that expand their input
    virtual ~Stage() {}
    // returns elements written; *consumed = input elements that need not be presented again
    virtual long process(csdr_amd_ctx *c, const void *d_in, size_t n_in, void *d_out, size_t out_cap, size_t *consumed) = 0;
    virtual size_t out_capacity(size_t n_in) { return n_in + 16; }
    virtual int next_bufsize(int b) { return b; }                   // what the reference passes to sendbufsize() for this command
    virtual const char *ctl_format() { return nullptr; }            // scanf format of a control line, if the command has a control channel
    virtual void retune(csdr_amd_ctx *, float, float) {}
    struct Control *ctl = nullptr;                                  // its open control channel (--fifo / --fd), polled in front of every pass (also inside `chain`)
};

struct Convert : Stage {
    int kind; int bigendian = 0;
    Convert(int k, size_t ie, size_t oe) : kind(k) { in_elem = ie; out_elem = oe; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        switch (kind) {
            case 0: MUST(csdr_amd_convert_u8_f(c, (const uint8_t *)i, (float *)o, n)); break;       // csdr.c:534-545
            case 1: MUST(csdr_amd_convert_f_u8(c, (const float *)i, (uint8_t *)o, n)); break;       // :546-557
            case 2: MUST(csdr_amd_convert_s8_f(c, (const int8_t *)i, (float *)o, n)); break;
            case 3: MUST(csdr_amd_convert_f_s8(c, (const float *)i, (int8_t *)o, n)); break;
            case 4: MUST(csdr_amd_convert_f_s16(c, (const float *)i, (int16_t *)o, n)); break;      // :582-593
            case 5: MUST(csdr_amd_convert_s16_f(c, (const int16_t *)i, (float *)o, n)); break;      // :594-605
            case 6: MUST(csdr_amd_convert_f_s24(c, (const float *)i, (uint8_t *)o, n, bigendian)); break;   // :606-619
            case 7: MUST(csdr_amd_convert_s24_f(c, (const uint8_t *)i, (float *)o, n, bigendian)); break;   // :620-633
        }
        return (long)n;
    }
};

struct Shift : Stage {   // csdr.c:703-925
    int variant; float rate; float phase = 0; int aux; bool real_in = false; CtxBuf<csdr_complexf> rot; size_t rot_cap = 0;
    Shift(int v, float r, int a) : variant(v), rate(r), aux(a) { in_elem = 8; out_elem = 8; granule = 1024; }
    const char *ctl_format() override { return (variant == CSDR_SHIFT_ADDITION || variant == CSDR_SHIFT_ADDFAST || variant == CSDR_SHIFT_UNROLL) ? "%g\n" : nullptr; }   // csdr.c:757-792, 808-843, 881-923, 3373-3407
    void retune(csdr_amd_ctx *, float r, float) override { rate = r; fprintf(stderr, "csdr %s: reinitialized to %g\n", g_cmd, r); }   // phase carries on (csdr.c:896-921)
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        if (real_in) {   // shift_addition_fc csdr.c:927-980
            if (!rot || n + 16 > rot_cap) { rot.reset(); rot_cap = n + 8192; rot = ctx_alloc<csdr_complexf>(c, 8 * rot_cap, "malloc"); }
            MUST(csdr_amd_rotator_generate(c, CSDR_SHIFT_ADDITION, rate, &phase, rot.get(), n, 1024, 0));
            MUST(csdr_amd_mix_fc(c, (const float *)i, (csdr_complexf *)o, rot.get(), 1, n, n, n));
        } else MUST(csdr_amd_shift_cc(c, variant, rate, &phase, (const csdr_complexf *)i, (csdr_complexf *)o, 1, n, n, n, 1024, aux));
        return (long)n;
    }
};

struct FirDecimate : Stage {   // csdr.c:1114-1177
    int D, ntaps; float *d_taps;
    FirDecimate(csdr_amd_ctx *c, int factor, float tbw, int window) : D(factor)
    {
        in_elem = 8; out_elem = 8;
        ntaps = csdr_amd_firdes_filter_len(tbw); min_block = (size_t)ntaps + factor;
        fprintf(stderr, "fir_decimate_cc: taps_length = %d\n", ntaps);
        std::vector<float> t(ntaps);
        csdr_amd_firdes_lowpass_f(t.data(), ntaps, 0.5f / (float)factor, window);
        d_taps = (float *)csdr_amd_malloc(c, 4 * ntaps);
        MUST(csdr_amd_h2d(c, d_taps, t.data(), 4 * ntaps));
    }
    size_t out_capacity(size_t n) override { return n / D + 16; }
    int next_bufsize(int b) override { return b / D; }               // csdr.c:1140
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        long no = csdr_amd_fir_decimate_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, 1, (int)n, n, cap, D, d_taps, ntaps);
        MUST(no);
        *cons = (size_t)no * D;                                    // the rest is re-presented (csdr.c:1172-1174)
        return no;
    }
};

struct Fmdemod : Stage {   // csdr.c:984-1012
    csdr_complexf *d_last;
    Fmdemod(csdr_amd_ctx *c) { in_elem = 8; out_elem = 4; d_last = (csdr_complexf *)csdr_amd_malloc(c, 8); MUST(csdr_amd_memset(c, d_last, 0, 8)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_fmdemod_quadri_cf(c, (const csdr_complexf *)i, (float *)o, 1, n, n, n, d_last)); return (long)n; }
};

struct Limit : Stage {   // csdr.c:673-686
    float m; Limit(float mm) : m(mm) { granule = 4; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_limit_ff(c, (const float *)i, (float *)o, n, m)); return (long)n; }
};

struct DeemphWfm : Stage {   // csdr.c:1014-1032
    float tau; int rate; float *d_last;
    DeemphWfm(csdr_amd_ctx *c, int r, float t) : tau(t), rate(r) { d_last = (float *)csdr_amd_malloc(c, 4); MUST(csdr_amd_memset(c, d_last, 0, 4)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_deemphasis_wfm_ff(c, (const float *)i, (float *)o, 1, n, n, n, tau, rate, d_last)); return (long)n; }
};

struct DeemphNfm : Stage {   // csdr.c:1068-1087
    // The reference's loop runs its FIR over the freshly allocated input buffer BEFORE it reads anything (`processed` starts at 0, so the
    // first fread is empty, csdr.c:1076-1081): its output is the FIR of  the_bufsize zeros ++ stream.  `pre` = zeros not yet consumed.
    int ntaps; float *d_taps; size_t pre; CtxBuf<float> d_tmp; size_t tmp_cap;
    DeemphNfm(csdr_amd_ctx *c, int rate, int the_bufsize) : pre((size_t)the_bufsize), tmp_cap(0)
    {
        const float *t = nullptr; ntaps = csdr_amd_nfm_deemph_taps(rate, &t); min_block = ntaps;
        if (!ntaps) { badsyntax("deemphasis_nfm_ff: invalid sample rate (this function works only with specific sample rates)."); exit(255); }
        d_taps = (float *)csdr_amd_malloc(c, 4 * ntaps); MUST(csdr_amd_h2d(c, d_taps, t, 4 * ntaps));
    }
    size_t out_capacity(size_t n) override { return n + pre + 16; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        if (!pre) {
            long no = csdr_amd_fir_ff(c, (const float *)i, (float *)o, 1, (int)n, n, cap, d_taps, ntaps);
            MUST(no); *cons = (size_t)no; return no;
        }
        const size_t tot = pre + n;
        if (tot > tmp_cap) { d_tmp.reset(); tmp_cap = tot + 64; d_tmp = ctx_alloc<float>(c, 4 * tmp_cap, "malloc"); }
        MUST(csdr_amd_memset(c, d_tmp.get(), 0, 4 * pre));
        if (n) MUST(csdr_amd_d2d(c, d_tmp.get() + pre, i, 4 * n));
        long no = csdr_amd_fir_ff(c, d_tmp.get(), (float *)o, 1, (int)tot, tot, cap, d_taps, ntaps);
        MUST(no);
        const size_t from_zeros = (size_t)no < pre ? (size_t)no : pre;
        pre -= from_zeros; *cons = (size_t)no - from_zeros;
        return no;
    }
};

struct FastAgc : Stage {   // csdr.c:1377-1406
    int block; float ref; float *d_state;
    FastAgc(csdr_amd_ctx *c, int b, float r) : block(b), ref(r)
    {
        granule = b; flush_partial = false; init_state(c, b);
    }
    int next_bufsize(int) override { return block; }                 // csdr.c:1386
    void init_state(csdr_amd_ctx *c, int b)
    {
        d_state = (float *)csdr_amd_malloc(c, 4 * (2 * (size_t)b + 4)); MUST(csdr_amd_memset(c, d_state, 0, 4 * (2 * (size_t)b + 4)));
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nb = (int)(n / block); *cons = (size_t)nb * block;
        if (nb) MUST(csdr_amd_fastagc_ff(c, (const float *)i, (float *)o, 1, nb, block, n, n, ref, d_state));
        return (long)nb * block;
    }
};

struct FracDec : Stage {   // csdr.c:1465-1525
    csdr_amd_fracdec *d; float rate;
    FracDec(float r, int points, const float *taps, int ntaps, int the_bufsize) : rate(r)
    {
        d = csdr_amd_fracdec_create(r, points, taps, ntaps); if (!d) { badsyntax(csdr_amd_last_error()); exit(255); }
        csdr_amd_fracdec_set_cli_bufsize(d, the_bufsize);                           // the reference's window loop: positions of inexact rates depend on it
        min_block = (size_t)the_bufsize;
    }
    size_t out_capacity(size_t n) override { return (size_t)(n / rate) + 64; }
    int next_bufsize(int b) override { return (int)(b / rate); }     // csdr.c:1497
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        int processed = 0;
        long no = csdr_amd_fractional_decimator_ff(c, d, (const float *)i, (float *)o, 1, (int)n, n, cap, &processed);
        MUST(no); *cons = processed > 0 ? (size_t)processed : 0; return no;
    }
};

struct Copy : Stage {   // csdr.c:1427, 1494: `rational_resampler_ff 1 1` and `fractional_decimator_ff 1` copy their input (inside `chain`; alone they become `clone`)
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; if (n) MUST(csdr_amd_d2d(c, o, i, 4 * n)); return (long)n; }
};

struct Resample : Stage {   // csdr.c:1409-1460: rational_resampler_ff over the_bufsize windows (the object replays the window loop, cap-exit repeats included)
    csdr_amd_resampler *r; int I, D;
    Resample(csdr_amd_ctx *c, int interpolation, int decimation, float tbw, int window, int the_bufsize) : I(interpolation), D(decimation)
    {
        const int nt = csdr_amd_firdes_filter_len(tbw);
        std::vector<float> t(nt);
        csdr_amd_rational_resampler_get_lowpass_f(t.data(), nt, I, D, window);
        r = csdr_amd_resampler_create(c, I, D, t.data(), nt, 1); if (!r) die("resampler_create");
        if (csdr_amd_resampler_set_cli_bufsize(r, the_bufsize) < 0) { badsyntax(csdr_amd_last_error()); exit(255); }
        min_block = (size_t)the_bufsize;
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_resampler_max_out(r, (long long)n) + 16; }
    int next_bufsize(int b) override { return (int)((long long)b * I / D); }       // csdr.c:1433
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        long long no = 0;
        MUST(csdr_amd_resampler_process(r, (const float *)i, (long long)n, n, (float *)o, cap, &no));
        *cons = n; return (long)no;
    }
};

struct Psk31 : Stage {   // simple_agc_cc csdr.c:2902-2930 | timing_recovery_cc csdr.c:2573-2648 | dbpsk_decoder_c_u8 csdr.c:3256-3268 | psk31_varicode_decoder_u8_u8
                        // csdr.c:2418-2431: one object for a consecutive run of them (`chain` fuses the run); the state lives on the device
    Owned<csdr_amd_psk31, csdr_amd_psk31_destroy> p; int first, last, extra, D; CtxBuf<int> d_count; CtxBuf<float> d_ex; size_t ex_cap;
    Psk31(csdr_amd_ctx *c, const csdr_amd_psk31_params &pr, int f, int l, int ex) : first(f), last(l), extra(ex), D(pr.decimation), ex_cap(0)
    {
        p.reset(csdr_amd_psk31_create(c, &pr, 1, f, l)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = f == CSDR_AMD_PSK31_VARICODE ? 1 : 8;
        out_elem = l <= CSDR_AMD_PSK31_TIMING ? (extra ? 4 : 8) : 1;
        d_count = ctx_alloc<int>(c, 64, "malloc");
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_psk31_max_out(p.get(), (long long)n) + 16; }
    int next_bufsize(int b) override { return (first <= CSDR_AMD_PSK31_TIMING && last >= CSDR_AMD_PSK31_TIMING) ? b / D : b; }     // csdr.c:2620
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        void *out = o; float *err = nullptr; unsigned *idx = nullptr;
        if (extra) {                                                   // --output_error / --output_indexes: the symbols go to a scratch buffer
            if (cap > ex_cap) { d_ex.reset(); ex_cap = cap + 64; d_ex = ctx_alloc<float>(c, 8 * ex_cap, "malloc"); }
            out = d_ex.get(); if (extra == 1) err = (float *)o; else idx = (unsigned *)o;
        }
        MUST(csdr_amd_psk31_process(p.get(), i, (long long)n, n, out, cap, d_count.get(), err, idx));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count.get(), sizeof k));
        return k;
    }
};

struct Psk31Tx : Stage {   // psk31_varicode_encoder_u8_u8 csdr.c:2780-2800 | differential_encoder_u8_u8 csdr.c:2816-2832 | psk_modulator_u8_c csdr.c:2684-2702 |
                          // psk31_interpolate_sine_cc csdr.c:2727-2747: one object for a consecutive run of them (`chain` fuses the run); the differential
                          // state and the shaper's last symbol live on the device.  The encoder is the library function applied to the whole stream.
    Owned<csdr_amd_psk31tx, csdr_amd_psk31tx_destroy> p; int first, last, I; CtxBuf<int> d_count;
    Psk31Tx(csdr_amd_ctx *c, int n_psk, int interpolation, int f, int l) : first(f), last(l), I(interpolation)
    {
        p.reset(csdr_amd_psk31tx_create(c, 1, n_psk, interpolation, f, l)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = f == CSDR_AMD_PSK31TX_SHAPE ? 8 : 1;
        out_elem = l >= CSDR_AMD_PSK31TX_MOD ? 8 : 1;
        d_count = ctx_alloc<int>(c, 64, "malloc");
        const size_t per_item = (size_t)csdr_amd_psk31tx_max_out(p.get(), 1) * out_elem;       // a pass writes at most 64 MiB
        max_block = std::max<size_t>(1024, ((size_t)64 << 20) / per_item / 1024 * 1024);
        if (f != l) fprintf(stderr, "csdr psk31_tx: one fused BPSK31 transmit object\n");
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_psk31tx_max_out(p.get(), (long long)n) + 16; }
    int next_bufsize(int b) override
    {   // csdr.c:2783 (x 8), :2734 (x interpolation); the two between keep it
        if (first == CSDR_AMD_PSK31TX_VARICODE) b *= 8;
        if (last == CSDR_AMD_PSK31TX_SHAPE) b *= I;
        return b;
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        MUST(csdr_amd_psk31tx_process(p.get(), i, (long long)n, nullptr, n, o, cap, d_count.get()));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count.get(), sizeof k));
        return k;
    }
};
struct DiffDecoder : Stage {   // differential_decoder_u8_u8 csdr.c:2816-2832: the previous byte on the device, 0 at the start
    CtxBuf<unsigned char> d_state;
    DiffDecoder(csdr_amd_ctx *c) { in_elem = 1; out_elem = 1; d_state = ctx_alloc<unsigned char>(c, 64, "malloc"); MUST(csdr_amd_memset(c, d_state.get(), 0, 64)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_differential_decoder_u8_u8(c, (const unsigned char *)i, (unsigned char *)o, 1, (long long)n, n, n, d_state.get())); return (long)n; }
};
struct DuplicateSamples : Stage {   // duplicate_samples_ntimes_u8_u8 csdr.c:2704-2725
    int ss, nt;
    DuplicateSamples(int sample_size, int ntimes) : ss(sample_size), nt(ntimes)
    { in_elem = 1; out_elem = 1; granule = (size_t)sample_size; flush_partial = false; max_block = std::max<size_t>(1024, ((size_t)64 << 20) / ntimes / 1024 * 1024); }
    size_t out_capacity(size_t n) override { return n * (size_t)nt + 16; }
    int next_bufsize(int b) override { return b * nt; }              // csdr.c:2714
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const size_t m = n / ss * ss; *cons = m;
        if (m) MUST(csdr_amd_duplicate_samples_ntimes_u8_u8(c, (const unsigned char *)i, (unsigned char *)o, 1, (long long)m, m, cap, ss, nt));
        return (long)(m * nt);
    }
};

struct Rtty : Stage {   // bfsk_demod_cf csdr.c:3271-3300 | serial_line_decoder_f_u8 csdr.c:2490-2528 | rtty_baudot2ascii_u8_u8 csdr.c:2461-2473: one object for a
                       // consecutive run of them (`chain` fuses the run); the complex history, the serial decoder's window remainder and the shift live on the device
    Owned<csdr_amd_rtty, csdr_amd_rtty_destroy> p; int first, last, B; CtxBuf<int> d_count;
    Rtty(csdr_amd_ctx *c, const csdr_amd_rtty_params &pr, int f, int l) : first(f), last(l), B(pr.cli_bufsize)
    {
        p.reset(csdr_amd_rtty_create(c, &pr, 1, f, l)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = f == CSDR_AMD_RTTY_BFSK ? 8 : f == CSDR_AMD_RTTY_SERIAL ? 4 : 1;
        out_elem = l == CSDR_AMD_RTTY_BFSK ? 4 : 1;
        d_count = ctx_alloc<int>(c, 64, "malloc");
        if (f != l) fprintf(stderr, "csdr rtty_rx: one fused RTTY receive object\n");
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_rtty_max_out(p.get(), (long long)n) + 16; }
    int next_bufsize(int b) override { return (first <= CSDR_AMD_RTTY_SERIAL && last >= CSDR_AMD_RTTY_SERIAL) ? B : b; }     // csdr.c:2506: its own (big) buffer
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        MUST(csdr_amd_rtty_process(p.get(), i, (long long)n, n, o, cap, d_count.get()));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count.get(), sizeof k));
        return k;
    }
};
struct RttyLine : Stage {   // rtty_line_decoder_u8_u8 csdr.c:2446-2458: rtty_baudot_decoder_push per byte, the decoder on the device
    csdr_amd_rtty_push_state *d_st; int *d_count;
    RttyLine(csdr_amd_ctx *c)
    {
        in_elem = 1; out_elem = 1;
        d_st = (csdr_amd_rtty_push_state *)csdr_amd_malloc(c, 256); d_count = (int *)(d_st + 4);
        if (!d_st) die("malloc");
        MUST(csdr_amd_memset(c, d_st, 0, 256));
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        MUST(csdr_amd_rtty_line_decoder_u8_u8(c, (const uint8_t *)i, (uint8_t *)o, 1, (long long)n, n, n, d_st, d_count));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count, sizeof k));
        return k;
    }
};
struct BinarySlicer : Stage {   // binary_slicer_f_u8 csdr.c:2475-2487
    BinarySlicer() { in_elem = 4; out_elem = 1; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_binary_slicer_f_u8(c, (const float *)i, (uint8_t *)o, 1, (long long)n, n, n)); return (long)n; }
};

// ---- the pulse-shaped symbol modem (modem.hip)
// pulse_shaping_filter_cc / firdes_pulse_shaping_filter_f (csdr.c:3159-3199): (RRC <samples_per_symbol> <num_taps> <beta> | COSINE <samples_per_symbol>), the checks in
// the reference's order; the designed taps into *taps.  false (message given) on bad syntax.
bool parse_pulse_filter(int argc, char **argv, std::vector<float> *taps)
{
    if (argc <= 2) { badsyntax("required parameter <pulse_shaping_filter_type> is missing."); return false; }
    const bool cosine = !strcmp(argv[2], "COSINE");                 // matched_filter_get_type_from_string: anything else is RRC
    int samples_per_symbol = 0, num_taps = 0; float beta = 0;
    if (argc <= 3) { badsyntax("required parameter <samples_per_symbol> is missing."); return false; }
    sscanf(argv[3], "%d", &samples_per_symbol);
    if (!cosine) {
        if (argc <= 4) { badsyntax("required parameter <num_taps> is missing."); return false; }
        sscanf(argv[4], "%d", &num_taps);
        if (argc <= 5) { badsyntax("required parameter <beta> is missing."); return false; }
        sscanf(argv[5], "%f", &beta);
    } else num_taps = 2 * samples_per_symbol + 1;
    if (samples_per_symbol <= 0) { badsyntax("samples_per_symbol should be >0"); return false; }
    if (num_taps <= 0 || (!cosine && num_taps % 2 == 0)) { badsyntax("num_taps should be odd (and >0)"); return false; }
    taps->assign(num_taps, 0.f);
    const int rc = cosine ? csdr_amd_firdes_cosine_f(taps->data(), num_taps, samples_per_symbol) : csdr_amd_firdes_rrc_f(taps->data(), num_taps, samples_per_symbol, beta);
    if (rc < 0) { badsyntax(csdr_amd_last_error()); return false; }
    return true;
}
bool parse_plain_interpolate(int argc, char **argv, int *interpolation)
{   // csdr.c:3238-3243
    if (argc <= 2) { badsyntax("required parameter <interpolation> is missing."); return false; }
    *interpolation = 0; sscanf(argv[2], "%d", interpolation);
    if (*interpolation <= 0) { badsyntax("interpolation should be >0"); return false; }
    return true;
}

struct PulseTx : Stage {   // [psk_modulator_u8_c n_psk |] plain_interpolate_cc I | pulse_shaping_filter_cc ...: one object for the run (`chain` fuses it); the symbols
                          // behind the last call live on the device.  The stream is the filter applied to the whole zero-stuffed stream.
    Owned<csdr_amd_pulsetx, csdr_amd_pulsetx_destroy> p; int I;
    PulseTx(csdr_amd_ctx *c, int n_psk, int interpolation, const std::vector<float> &taps, int f) : I(interpolation)
    {
        p.reset(csdr_amd_pulsetx_create(c, 1, n_psk, interpolation, taps.data(), (int)taps.size(), f, CSDR_AMD_PULSETX_SHAPE)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = f == CSDR_AMD_PULSETX_SHAPE ? 8 : 1; out_elem = 8;
        max_block = std::max<size_t>(1024, ((size_t)64 << 20) / ((size_t)interpolation * out_elem) / 1024 * 1024);       // a pass writes at most 64 MiB
        fprintf(stderr, "csdr pulse_tx: one fused pulse-shaping transmit object\n");
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_pulsetx_max_out(p.get(), (long long)n) + 16; }
    int next_bufsize(int b) override { return b * I; }               // csdr.c:3243
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        long long k = 0;
        MUST(csdr_amd_pulsetx_process(p.get(), i, (long long)n, n, o, cap, &k));
        return (long)k;
    }
};
struct PlainInterpolate : Stage {   // plain_interpolate_cc csdr.c:3238-3254
    int I;
    PlainInterpolate(int interpolation) : I(interpolation)
    { in_elem = 8; out_elem = 8; max_block = std::max<size_t>(1024, ((size_t)64 << 20) / ((size_t)interpolation * 8) / 1024 * 1024); }
    size_t out_capacity(size_t n) override { return n * (size_t)I + 16; }
    int next_bufsize(int b) override { return b * I; }               // csdr.c:3243
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    { *cons = n; MUST(csdr_amd_plain_interpolate_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, 1, (long long)n, n, cap, I)); return (long)(n * I); }
};
struct PulseFilter : Stage {   // pulse_shaping_filter_cc csdr.c:3159-3219: apply_real_fir_cc over the stream, the unconsumed tail presented again
    int ntaps; CtxBuf<float> d_taps;
    PulseFilter(csdr_amd_ctx *c, const std::vector<float> &taps) : ntaps((int)taps.size())
    {
        in_elem = 8; out_elem = 8; min_block = (size_t)ntaps;
        d_taps = ctx_alloc<float>(c, 4 * taps.size(), "malloc");
        MUST(csdr_amd_h2d(c, d_taps.get(), taps.data(), 4 * taps.size()));
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const long no = csdr_amd_apply_real_fir_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, 1, (int)n, n, cap, d_taps.get(), ntaps);
        MUST(no);
        *cons = (size_t)no;                                        // the rest is re-presented (csdr.c:3216-3217)
        return no;
    }
};
struct PeaksFir : Stage {   // peaks_fir_cc csdr.c:2975-3016: apply_fir_cc over the stream with the taps of its peak rates, the unconsumed tail (taps_length - 1
                           // samples) presented again: the valid filter output of the whole stream, whatever the block size
    int ntaps; CtxBuf<csdr_complexf> d_taps;
    PeaksFir(csdr_amd_ctx *c, int taps_length, const std::vector<float> &rates) : ntaps(taps_length)
    {
        in_elem = 8; out_elem = 8; min_block = (size_t)ntaps;
        std::vector<csdr_complexf> taps((size_t)ntaps);
        csdr_amd_firdes_peaks_c(taps.data(), ntaps, rates.data(), (int)rates.size(), CSDR_WINDOW_HAMMING);      // WINDOW_DEFAULT, csdr.c:2991
        d_taps = ctx_alloc<csdr_complexf>(c, 8 * taps.size(), "malloc");
        MUST(csdr_amd_h2d(c, d_taps.get(), taps.data(), 8 * taps.size()));
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const long no = n >= (size_t)ntaps ? (long)(n - ntaps + 1) : 0;
        MUST(csdr_amd_apply_fir_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, 1, (long long)n, n, cap, d_taps.get(), 0, ntaps, 0));
        *cons = (size_t)no;                                        // the rest is re-presented (csdr.c:3013-3014)
        return no;
    }
};
struct PulseRx : Stage {   // pulse_shaping_filter_cc ... | timing_recovery_cc ... [[| realpart_cf] | gain_ff g | generic_slicer_f_u8 n]: one object for the run (`chain` fuses
                          // it); the unconsumed tail and the loop's state live on the device.  The filter is evaluated only where the timing loop reads it.
    Owned<csdr_amd_pulserx, csdr_amd_pulserx_destroy> p; int D; CtxBuf<int> d_count;
    PulseRx(csdr_amd_ctx *c, const csdr_amd_pulserx_params &pr, int last) : D(pr.decimation)
    {
        p.reset(csdr_amd_pulserx_create(c, &pr, 1, CSDR_AMD_PULSERX_FILTER, last)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = 8; out_elem = last == CSDR_AMD_PULSERX_TIMING ? 8 : 1;
        d_count = ctx_alloc<int>(c, 64, "malloc");
        fprintf(stderr, "csdr pulse_rx: one fused pulse-shaped receive object\n");
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_pulserx_max_out(p.get(), (long long)n) + 16; }
    int next_bufsize(int b) override { return b / D; }               // csdr.c:2620 (the other commands of the run pass their buffer size on)
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        MUST(csdr_amd_pulserx_process(p.get(), (const csdr_complexf *)i, (long long)n, n, o, cap, d_count.get(), nullptr, nullptr));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count.get(), sizeof k));
        return k;
    }
};
struct FrameSync : Stage {   // pattern_search_u8_u8 csdr.c:3532-3597: one device searcher for the run; ring, index and the open payload live on the device between passes.
                            // Everything handed in is consumed; what comes out is the payload bytes that arrived (no stale block, no end-of-file byte at EOF).
    Owned<csdr_amd_framesync, csdr_amd_framesync_destroy> p; CtxBuf<int> d_count;
    FrameSync(csdr_amd_ctx *c, const std::vector<unsigned> &pattern, int values_after, int max_mismatch)
    {
        csdr_amd_framesync *h = nullptr;
        if (csdr_amd_framesync_create(c, 1, pattern.data(), (int)pattern.size(), values_after, max_mismatch, &h) < 0) { badsyntax(csdr_amd_last_error()); exit(255); }
        p.reset(h);
        in_elem = 1; out_elem = 1;
        d_count = ctx_alloc<int>(c, 64, "malloc");
        fprintf(stderr, "csdr pattern_search_u8_u8: one device frame synchroniser (%d pattern values, %d after, %d may differ)\n", (int)pattern.size(), values_after, max_mismatch);
    }
    int next_bufsize(int) override { return 1; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        MUST(csdr_amd_framesync_process(p.get(), (const uint8_t *)i, n, (long long)n, nullptr, (uint8_t *)o, cap, d_count.get(), nullptr, 0, nullptr));
        int k = 0; MUST(csdr_amd_d2h(c, &k, d_count.get(), sizeof k));
        return k;
    }
};
struct GenericSlicer : Stage {   // generic_slicer_f_u8 csdr.c:3221-3236
    int n_symbols;
    GenericSlicer(int n) : n_symbols(n) { in_elem = 4; out_elem = 1; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_generic_slicer_f_u8(c, (const float *)i, (uint8_t *)o, 1, (long long)n, n, n, n_symbols)); return (long)n; }
};
struct PackBits : Stage {   // pack_bits_1to8_u8_u8 csdr.c:2749-2763 (a byte -> 8 bytes) / pack_bits_8to1_u8_u8 csdr.c:2765-2778 (8 bytes -> a byte; a partial group at EOF is dropped)
    bool expand;
    PackBits(bool e) : expand(e)
    { in_elem = 1; out_elem = 1; if (!e) { granule = 8; flush_partial = false; } else max_block = (size_t)8 << 20; }
    size_t out_capacity(size_t n) override { return (expand ? 8 * n : n / 8) + 16; }
    int next_bufsize(int b) override { return expand ? b * 8 : 1; }  // csdr.c:2752, 2768
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        if (expand) { *cons = n; MUST(csdr_amd_pack_bits_1to8_u8_u8(c, (const uint8_t *)i, (uint8_t *)o, 1, (long long)n, n, cap)); return (long)(8 * n); }
        const size_t m = n / 8 * 8; *cons = m;
        if (m) MUST(csdr_amd_pack_bits_8to1_u8_u8(c, (const uint8_t *)i, (uint8_t *)o, 1, (long long)m, m, cap));
        return (long)(m / 8);
    }
};

struct Squelch : Stage {   // squelch_and_smeter_cc csdr.c:2192-2243: blocks of the_bufsize samples counted from the start of the stream, however many a pass moves;
                          // a new level (control channel, polled in front of every pass) applies from the next block; block k's power goes to the out fifo as "%g\n"
                          // when k mod (report_every_nth + 2) == report_every_nth + 1, written non-blocking as the reference does
    Owned<csdr_amd_squelch, csdr_amd_squelch_destroy> p; int B, every, fd_out; size_t max_blocks; CtxBuf<float> d_power; std::vector<float> h_power;
    Squelch(csdr_amd_ctx *c, int the_bufsize, int use_every_nth, int report_every_nth, float level, int out_fd, size_t block) : B(the_bufsize), every(report_every_nth), fd_out(out_fd)
    {
        in_elem = 8; out_elem = 8; granule = (size_t)the_bufsize; flush_partial = false;
        const size_t most = (block > 4 * granule ? block : 4 * granule) + granule + 64;      // the largest pass run() hands this stage
        p.reset(csdr_amd_squelch_create(c, 1, the_bufsize, use_every_nth, &level, (long long)most)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        max_blocks = (size_t)csdr_amd_squelch_max_blocks(p.get());
        d_power = ctx_alloc<float>(c, 4 * max_blocks + 64, "malloc"); h_power.resize(max_blocks);
    }
    const char *ctl_format() override { return "%g\n"; }
    void retune(csdr_amd_ctx *, float level, float) override { MUST(csdr_amd_squelch_set_level(p.get(), 0, level)); fprintf(stderr, "csdr %s: new squelch level is %g\n", g_cmd, level); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const size_t nb = n / B; *cons = nb * B;
        if (!nb) return 0;
        const long long k0 = csdr_amd_squelch_block_index(p.get(), 0);
        MUST(csdr_amd_squelch_process(p.get(), (const csdr_complexf *)i, (long long)(nb * B), n, (csdr_complexf *)o, cap, d_power.get(), max_blocks, nullptr, nullptr));
        bool any = false;
        for (size_t k = 0; k < nb && !any; k++) any = csdr_amd_squelch_report_due(every, k0 + (long long)k) != 0;
        if (any && fd_out >= 0) {
            MUST(csdr_amd_d2h(c, h_power.data(), d_power.get(), 4 * nb));
            for (size_t k = 0; k < nb; k++) if (csdr_amd_squelch_report_due(every, k0 + (long long)k)) {
                char line[101]; const int len = snprintf(line, 100, "%g\n", h_power[k]);
                (void)!write(fd_out, line, (size_t)len);                 // non-blocking: a full fifo drops the line (csdr.c:2211-2228)
            }
        }
        return (long)(nb * B);
    }
};

struct Carrier : Stage {   // bpsk_costas_loop_cc csdr.c:2834-2899 | pll_cc csdr.c:2532-2571: one sample out per sample in, the loop state on the device; every pass, the
                          // stream's last partial one included, is processed whole (as the simple_agc_cc stage)
    enum { OUT = 0, ERROR = 1, DPHASE = 2, NCO = 3, COMBINED = 4 };
    Owned<csdr_amd_carrier, csdr_amd_carrier_destroy> p; int which; FILE *files[3]; CtxBuf<char> d_side; size_t side_cap = 0; std::vector<char> h_side;
    Carrier(csdr_amd_ctx *c, const csdr_amd_carrier_params &pr, int w, FILE *f_error = nullptr, FILE *f_dphase = nullptr, FILE *f_nco = nullptr) : which(w)
    {
        files[0] = f_error; files[1] = f_dphase; files[2] = f_nco;
        p.reset(csdr_amd_carrier_create(c, &pr, 1)); if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        in_elem = 8; out_elem = (w == ERROR || w == DPHASE) ? 4 : 8;
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        if (!n) return 0;
        const csdr_complexf *x = (const csdr_complexf *)i;
        if (which != COMBINED) {
            MUST(csdr_amd_carrier_process(p.get(), x, (long long)n, n, which == OUT ? (csdr_complexf *)o : nullptr, which == ERROR ? (float *)o : nullptr,
                                          which == DPHASE ? (float *)o : nullptr, which == NCO ? (csdr_complexf *)o : nullptr, n));
            return (long)n;
        }
        // --output_combined: the samples to stdout; error, dphase and nco to their files (csdr.c:2887-2893).  One side buffer: nco (8 n bytes), error, dphase (4 n each)
        if (n > side_cap) { d_side.reset(); side_cap = n + 8192; d_side = ctx_alloc<char>(c, 16 * side_cap, "malloc"); h_side.resize(16 * side_cap); }
        csdr_complexf *d_nco = (csdr_complexf *)d_side.get(); float *d_err = (float *)(d_nco + n), *d_dph = d_err + n;
        MUST(csdr_amd_carrier_process(p.get(), x, (long long)n, n, (csdr_complexf *)o, d_err, d_dph, d_nco, n));
        MUST(csdr_amd_d2h(c, h_side.data(), d_side.get(), 16 * n));
        fwrite(h_side.data() + 8 * n, 4, n, files[0]); fwrite(h_side.data() + 12 * n, 4, n, files[1]); fwrite(h_side.data(), 8, n, files[2]);
        for (FILE *f : files) fflush(f);
        return (long)n;
    }
};

struct Interp : Stage {   // csdr.c:1179-1232: fir_interpolate_cc over the_bufsize windows, the first over a buffer of zeros
    csdr_amd_interp *p; int I;
    Interp(csdr_amd_ctx *c, int factor, float tbw, int window, int the_bufsize) : I(factor)
    {
        in_elem = 8; out_elem = 8;
        const int nt = csdr_amd_firdes_filter_len(tbw);
        fprintf(stderr, "csdr fir_interpolate_cc: taps_length = %d\n", nt);
        std::vector<float> t(nt);
        csdr_amd_firdes_lowpass_f(t.data(), nt, 0.5f / (float)factor, window);
        p = csdr_amd_interp_create(c, factor, t.data(), nt, 1); if (!p) die("interp_create");
        MUST(csdr_amd_interp_set_cli_bufsize(p, the_bufsize));
        min_block = (size_t)nt;
    }
    size_t out_capacity(size_t n) override { return (size_t)csdr_amd_interp_max_out(p, (long long)n) + 16; }
    int next_bufsize(int b) override { return b * I; }                            // csdr.c:1207
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        long long no = 0;
        MUST(csdr_amd_interp_process(p, (const csdr_complexf *)i, (long long)n, n, (csdr_complexf *)o, cap, &no));
        *cons = n; return (long)no;
    }
};

struct Bandpass : Stage {   // csdr.c:1810-1886
    csdr_amd_fftfilt *f; int inp; int n_taps, win;
    const char *ctl_format() override { return "%g %g\n"; }
    void retune(csdr_amd_ctx *, float lo, float hi) override       // new band edges, the overlap carries on (csdr.c:1862-1880)
    {
        fprintf(stderr, "csdr bandpass_fir_fft_cc: filter initialized, low_cut = %g, high_cut = %g\n", lo, hi);
        std::vector<csdr_complexf> t(n_taps);
        csdr_amd_firdes_bandpass_c(t.data(), n_taps, lo, hi, win);
        MUST(csdr_amd_fftfilt_set_taps(f, t.data(), n_taps));
    }
    Bandpass(csdr_amd_ctx *c, float lo, float hi, float tbw, int window, size_t block)
    {
        in_elem = 8; out_elem = 8; flush_partial = false;
        const int ntaps = csdr_amd_firdes_filter_len(tbw); n_taps = ntaps; win = window;
        int fft = csdr_amd_next_pow2(ntaps);
        if (fft - ntaps < 200) fft <<= 1;                                            // csdr.c:1834-1836
        inp = fft - ntaps + 1;
        fprintf(stderr, "csdr bandpass_fir_fft_cc: (fft_size = %d) = (taps_length = %d) + (input_size = %d) - 1\n(overlap_length = %d) = taps_length - 1\n", fft, ntaps, inp, ntaps - 1);
        std::vector<csdr_complexf> t(ntaps);
        csdr_amd_firdes_bandpass_c(t.data(), ntaps, lo, hi, window);
        f = csdr_amd_fftfilt_create(c, fft, t.data(), ntaps, 1, (int)(block / inp + 2));
        if (!f) die("fftfilt_create");
        granule = inp;
    }
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nb = (int)(n / inp); *cons = (size_t)nb * inp;
        if (nb) MUST(csdr_amd_fftfilt_process(f, (const csdr_complexf *)i, (csdr_complexf *)o, nb, n, n));
        return (long)nb * inp;
    }
};

struct DdcFwd : Stage {   // csdr.c:2255-2300
    csdr_amd_fastddc_fwd *f; csdr_fastddc_t ddc;
    DdcFwd(csdr_amd_ctx *c, int D, float tbw, size_t block)
    {
        in_elem = 8; out_elem = 8; flush_partial = false;
        if (csdr_amd_fastddc_init(&ddc, tbw, D, 0)) { badsyntax("error in fastddc_init()"); exit(1); }
        f = csdr_amd_fastddc_fwd_create(c, &ddc, (int)(block / ddc.input_size + 2)); if (!f) die("fastddc_fwd_create");
        granule = ddc.input_size;
    }
    size_t out_capacity(size_t n) override { return (n / ddc.input_size + 1) * (size_t)ddc.fft_size; }
    int next_bufsize(int) override { return ddc.fft_size; }          // csdr.c:2274
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nb = (int)(n / ddc.input_size); *cons = (size_t)nb * ddc.input_size;
        if (nb) MUST(csdr_amd_fastddc_fwd_process(f, (const csdr_complexf *)i, (csdr_complexf *)o, nb));
        return (long)nb * ddc.fft_size;
    }
};

struct DdcInv : Stage {   // csdr.c:2302-2378
    csdr_amd_fastddc_inv *f = nullptr; csdr_fastddc_t ddc; int maxb, dec, win; float tbw_;
    void build(csdr_amd_ctx *c, float shift)                         // the reference rebuilds everything on a retune, status included (csdr.c:2329-2376)
    {
        if (f) csdr_amd_fastddc_inv_destroy(f);
        if (csdr_amd_fastddc_init(&ddc, tbw_, dec, shift)) { badsyntax("error in fastddc_init()"); exit(1); }
        f = csdr_amd_fastddc_inv_create(c, tbw_, dec, &shift, 1, win, maxb); if (!f) die("fastddc_inv_create");
    }
    const char *ctl_format() override { return "%g\n"; }
    void retune(csdr_amd_ctx *c, float shift, float) override { build(c, shift); }
    int next_bufsize(int) override { return ddc.post_input_size / ddc.post_decimation; }   // csdr.c:2339
    DdcInv(csdr_amd_ctx *c, float shift, int D, float tbw, int window, size_t block) : dec(D), win(window), tbw_(tbw)
    {
        in_elem = 8; out_elem = 8; flush_partial = false;
        if (csdr_amd_fastddc_init(&ddc, tbw, D, shift)) { badsyntax("error in fastddc_init()"); exit(1); }
        maxb = (int)(block / ddc.fft_size + 2);
        build(c, shift);
        granule = ddc.fft_size;
    }
    size_t out_capacity(size_t n) override { return (n / ddc.fft_size + 1) * (size_t)(ddc.post_input_size / ddc.post_decimation + 2) + 16; }
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const int nb = (int)(n / ddc.fft_size); *cons = (size_t)nb * ddc.fft_size;
        int count = 0;
        if (nb) MUST(csdr_amd_fastddc_inv_process(f, (const csdr_complexf *)i, nb, (csdr_complexf *)o, cap, &count));
        return count;
    }
};

struct WfmChain : Stage {   // the fused README.md:66 chain as ONE command (extension: not in the reference's command list)
    csdr_amd_wfm *w; bool retunable;
    const char *ctl_format() override { return retunable ? "%g\n" : nullptr; }       // `wfm_chain_u8_s16 --fifo <path>`: the shift stage's control channel (csdr.c:881-923)
    void retune(csdr_amd_ctx *, float r, float) override { MUST(csdr_amd_wfm_set_rate(w, 0, r)); fprintf(stderr, "csdr %s: reinitialized to %g\n", g_cmd, r); }
    WfmChain(csdr_amd_ctx *c, float shift, size_t block, bool with_ctl) : retunable(with_ctl)
    {
        in_elem = 2; out_elem = 2; granule = 1024;
        std::vector<float> t(79);
        const int nt = csdr_amd_firdes_filter_len(0.05f);
        t.resize(nt); csdr_amd_firdes_lowpass_f(t.data(), nt, 0.05f, CSDR_WINDOW_HAMMING);
        // The rate-per-stream object, always: its one stream can be retuned between two calls (control channel), and its kernel spreads ONE stream over the 16 columns of
        // a tile (16 time segments) where the shared-rate kernel fills one of 16 -- a 4 M-sample block took the latter 0.41 ms, 10 GS/s before a byte was read
        // (CSDR_AMD_CLI_TIMING, round 5).  CSDR_AMD_CLI_SHARED=1: the shared-rate object as before.
        // Blocks under 1 Mi samples stay on the shared-rate object (256 Ki: 3.8 against 2.5 GS/s: per call the rate-per-stream object also looks its seeds up).
        w = (with_ctl || (block >= (1u << 20) && !getenv("CSDR_AMD_CLI_SHARED"))) ? csdr_amd_wfm_create_rates(c, 1, &shift, 10, t.data(), nt, 5, 50e-6f, 48000, block + 1024)
                                                         : csdr_amd_wfm_create(c, 1, shift, 10, t.data(), nt, 5, 50e-6f, 48000, block + 1024);
        if (!w) die("wfm_create");
        if (csdr_amd_wfm_fallback(w)) fprintf(stderr, "csdr %s: note: this shape runs on the fallback kernels (k_wfm_front + k_wfm_back), not on the matrix-core chain kernel\n", g_cmd);
    }
    size_t out_capacity(size_t n) override { return n / 50 + 64; }
    int next_bufsize(int b) override { return b / 50; }
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {   // (one stream: the pitch only has to satisfy the 16-byte rule -- a stream's last block can have any length)
        *cons = n; long na = csdr_amd_wfm_process(w, (const uint8_t *)i, (2 * n + 127) & ~(size_t)127, n, (int16_t *)o, nullptr, cap); MUST(na); return na; }
};

// `CSDR_AMD_RESIDENT=1 csdr wfm_chain_u8_s16 <shift_rate>`: the same chain through the RESIDENT form (csdr_amd_wfm_ring_*): one persistent grid walks a ring of
// the reference's own blocks -- 16384 samples per read, csdr.c:189-193, 330-392 -- , no kernel launch per block; a live stream (a block every 6.8 ms at 2.4 MS/s) keeps
// the grid on the GPU between blocks (idle time 20 ms), a stalled one lets it go.  Whole blocks only: what is left of the stream behind its last whole block is dropped at
// EOF, as the reference's stages drop a partial the_bufsize read (csdr.c:232-247).
struct WfmRingStage : Stage {
    csdr_amd_wfm_ring *r; size_t T; bool retunable;
    const char *ctl_format() override { return retunable ? "%g\n" : nullptr; }
    void retune(csdr_amd_ctx *, float rt, float) override { MUST(csdr_amd_wfm_ring_set_rate(r, rt)); fprintf(stderr, "csdr %s: reinitialized to %g\n", g_cmd, rt); }
    WfmRingStage(csdr_amd_ctx *c, float shift, bool with_ctl) : T(16384), retunable(with_ctl)
    {
        in_elem = 2; out_elem = 2; granule = T; flush_partial = false; min_block = T / 4;
        const int nt = csdr_amd_firdes_filter_len(0.05f);
        std::vector<float> t(nt); csdr_amd_firdes_lowpass_f(t.data(), nt, 0.05f, CSDR_WINDOW_HAMMING);
        r = csdr_amd_wfm_ring_create(c, 1, shift, 10, t.data(), nt, 5, 50e-6f, 48000, T, 8);
        if (!r) die("wfm_ring_create");
        MUST(csdr_amd_wfm_ring_set_timeouts(r, 20000.0, 1000.0));
        fprintf(stderr, "csdr %s: resident grid (%d workgroups), ring of %d blocks of %zu samples\n", g_cmd, csdr_amd_wfm_ring_grid(r), csdr_amd_wfm_ring_slots(r), T);
    }
    ~WfmRingStage() { csdr_amd_wfm_ring_destroy(r); }
    size_t out_capacity(size_t n) override { return n / 50 + 64; }
    int next_bufsize(int b) override { return b / 50; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        const size_t nb = n / T; *cons = nb * T;
        const int depth = csdr_amd_wfm_ring_slots(r) - 2;
        long total = 0;
        for (size_t b0 = 0; b0 < nb; b0 += depth) {                  // groups of as many blocks as the ring holds in flight: inputs in, posted, collected in order
            const size_t nbk = nb - b0 < (size_t)depth ? nb - b0 : (size_t)depth;
            const long long s0 = csdr_amd_wfm_ring_submitted(r);
            for (size_t b = 0; b < nbk; b++) {
                MUST(csdr_amd_wfm_ring_acquire(r, s0 + (long long)b, 0));
                size_t pitch; uint8_t *slot = csdr_amd_wfm_ring_input(r, s0 + (long long)b, &pitch);
                MUST(csdr_amd_d2d(c, slot, (const uint8_t *)i + 2 * T * (b0 + b), 2 * T));
            }
            MUST(csdr_amd_ctx_sync(c));                              // the blocks lie in their slots before they are posted
            for (size_t b = 0; b < nbk; b++) { const long long k = csdr_amd_wfm_ring_submit(r); MUST((int)(k < 0 ? k : 0)); }
            for (size_t b = 0; b < nbk; b++) {
                const long na = csdr_amd_wfm_ring_wait(r, s0 + (long long)b, 0); MUST((int)(na < 0 ? na : 0));
                if ((size_t)(total + na) > cap) die("wfm ring: output buffer too small");
                size_t op; const int16_t *out = csdr_amd_wfm_ring_output(r, s0 + (long long)b, &op);
                MUST(csdr_amd_d2d(c, (int16_t *)o + total, out, 2 * (size_t)na));
                total += na;
            }
        }
        return total;
    }
};

struct DdcFront : Stage {   // convert_u8_f | shift_addition_cc r | fir_decimate_cc D tbw window as ONE command (extension): the head of the NFM / AM / SSB chains
    csdr_amd_ddc *d; int dec; bool retunable;
    const char *ctl_format() override { return retunable ? "%g\n" : nullptr; }
    void retune(csdr_amd_ctx *, float r, float) override { MUST(csdr_amd_ddc_set_rate(d, 0, r)); fprintf(stderr, "csdr %s: reinitialized to %g\n", g_cmd, r); }
    DdcFront(csdr_amd_ctx *c, float shift, int D, float tbw, int window, size_t block, bool with_ctl) : dec(D), retunable(with_ctl)
    {
        in_elem = 2; out_elem = 8; granule = 1024;
        const int nt = csdr_amd_firdes_filter_len(tbw);
        std::vector<float> t(nt); csdr_amd_firdes_lowpass_f(t.data(), nt, 0.5f / (float)D, window);       // csdr.c:1144-1158
        d = with_ctl ? csdr_amd_ddc_create_rates(c, 1, &shift, D, t.data(), nt, block + 1024) : csdr_amd_ddc_create(c, 1, shift, D, t.data(), nt, block + 1024);
        if (!d) die("ddc_create");
    }
    size_t out_capacity(size_t n) override { return n / dec + 64; }
    int next_bufsize(int b) override { return b / dec; }
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n; long no = csdr_amd_ddc_process(d, (const uint8_t *)i, (2 * n + 127) & ~(size_t)127, n, (csdr_complexf *)o, cap); MUST(no);
        if (!noted && n >= 4096 && csdr_amd_ddc_fallback(d)) { noted = true; fprintf(stderr, "csdr %s: note: this shape runs on the plain kernel (k_ddc_direct), not on the matrix-core front end\n", g_cmd); }
        return no;
    }
    bool noted = false;
};

struct NfmChain : Stage {   // the README.md:87 chain as ONE command (extension)
    csdr_amd_nfm *w; int dec; bool retunable;
    const char *ctl_format() override { return retunable ? "%g\n" : nullptr; }
    void retune(csdr_amd_ctx *, float r, float) override { MUST(csdr_amd_nfm_set_rate(w, 0, r)); fprintf(stderr, "csdr %s: reinitialized to %g\n", g_cmd, r); }
    NfmChain(csdr_amd_ctx *c, float shift, int D, float tbw, size_t block, bool with_ctl) : dec(D), retunable(with_ctl)
    {
        in_elem = 2; out_elem = 2; granule = 1024;
        const int nt = csdr_amd_firdes_filter_len(tbw);
        std::vector<float> t(nt); csdr_amd_firdes_lowpass_f(t.data(), nt, 0.5f / (float)D, CSDR_WINDOW_HAMMING);
        w = (with_ctl || (block >= (1u << 20) && !getenv("CSDR_AMD_CLI_SHARED"))) ? csdr_amd_nfm_create_rates(c, 1, &shift, D, t.data(), nt, 48000, 1024, 1.0f, 1.0f, block + 1024)      // (as WfmChain)
                     : csdr_amd_nfm_create(c, 1, shift, D, t.data(), nt, 48000, 1024, 1.0f, 1.0f, block + 1024);      // fastagc_ff defaults csdr.c:1379-1391
        if (!w) die("nfm_create");
    }
    size_t out_capacity(size_t n) override { return n / dec + 4096; }
    int next_bufsize(int b) override { return b / dec; }
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n; long na = csdr_amd_nfm_process(w, (const uint8_t *)i, (2 * n + 127) & ~(size_t)127, n, (int16_t *)o, nullptr, cap); MUST(na);
        if (!noted && n >= 4096 && csdr_amd_ddc_fallback(csdr_amd_nfm_front_end(w))) { noted = true; fprintf(stderr, "csdr %s: note: the front end of this shape runs on the plain kernel (k_ddc_direct), not on the matrix-core kernel\n", g_cmd); }
        return na;
    }
    bool noted = false;
};

struct NfmRx : Stage {   // fmdemod_quadri_cf | limit_ff | deemphasis_nfm_ff <audio_rate> | fastagc_ff | convert_f_s16 as ONE command (extension): the stage behind one fastddc_inv_cc,
                        // one channel of csdr_amd_fmrx; the filter's unconsumed input, the previous sample and the AGC's blocks stay in the object between passes
                        // --squelch: squelch_and_smeter_cc in front, inside the object (csdr_amd_fmrx_create_squelched): blocks of the_bufsize samples, the level
                        // protocol and the "%g\n" reports of that command (csdr.c:2205-2240), so `squelch_and_smeter_cc ... | nfm_rx_cc_s16` as one process
    Owned<csdr_amd_fmrx, csdr_amd_fmrx_destroy> p; size_t max_n; int sqB = 0, every = 0, fd_out = -1; size_t max_blocks = 0; CtxBuf<float> d_power; std::vector<float> h_power;
    NfmRx(csdr_amd_ctx *c, int audio_rate, size_t block) : max_n(block + 1024)
    {
        in_elem = 8; out_elem = 2;
        p.reset(csdr_amd_fmrx_create(c, 1, audio_rate, 1024, 1.0f, 1.0f, max_n));      // limit_ff and fastagc_ff defaults (csdr.c:673-686, 1379-1391)
        if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
    }
    NfmRx(csdr_amd_ctx *c, int audio_rate, size_t block, int squelch_block, int use_every_nth, int report_every_nth, float level, int out_fd)
        : max_n(block + 1024), sqB(squelch_block), every(report_every_nth), fd_out(out_fd)
    {
        in_elem = 8; out_elem = 2;
        p.reset(csdr_amd_fmrx_create_squelched(c, 1, audio_rate, 1024, 1.0f, 1.0f, max_n, squelch_block, use_every_nth, &level));
        if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        max_blocks = max_n / (size_t)squelch_block + 1;
        d_power = ctx_alloc<float>(c, 4 * max_blocks + 64, "malloc"); h_power.resize(max_blocks);
    }
    size_t out_capacity(size_t n) override { return n + 4096 + (size_t)sqB; }
    const char *ctl_format() override { return sqB ? "%g\n" : nullptr; }
    void retune(csdr_amd_ctx *, float level, float) override { MUST(csdr_amd_fmrx_set_squelch_level(p.get(), 0, level)); fprintf(stderr, "csdr %s: new squelch level is %g\n", g_cmd, level); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        long total = 0;
        for (size_t at = 0; at < n; at += max_n) {                     // (inside `chain` a pass may hand over more than the command's own block)
            const size_t m = std::min(max_n, n - at);
            if (!sqB) {
                const long long na = csdr_amd_fmrx_process(p.get(), (const csdr_complexf *)i + at, 0, (long long)m, (int16_t *)o + total, nullptr, cap - total);
                MUST(na);
                total += (long)na;
                continue;
            }
            const long long k0 = csdr_amd_fmrx_squelch_block_index(p.get());
            int nb = 0;
            const long long na = csdr_amd_fmrx_process_squelched(p.get(), (const csdr_complexf *)i + at, 0, (long long)m, (int16_t *)o + total, nullptr, cap - total, d_power.get(),
                                                                 max_blocks, nullptr, &nb);
            MUST(na);
            total += (long)na;
            bool any = false;
            for (int k = 0; k < nb && !any; k++) any = csdr_amd_squelch_report_due(every, k0 + k) != 0;
            if (any && fd_out >= 0) {
                MUST(csdr_amd_d2h(c, h_power.data(), d_power.get(), 4 * (size_t)nb));
                for (int k = 0; k < nb; k++) if (csdr_amd_squelch_report_due(every, k0 + k)) {
                    char line[101]; const int len = snprintf(line, 100, "%g\n", h_power[k]);
                    (void)!write(fd_out, line, (size_t)len);             // non-blocking: a full fifo drops the line (csdr.c:2211-2228)
                }
            }
        }
        return total;
    }
};

struct WfmRxStage : Stage {   // fmdemod_quadri_cf | fractional_decimator_ff <rate> | deemphasis_wfm_ff <audio_rate> <tau> | convert_f_s16 as ONE command (extension): the stage behind
                             // one fastddc_inv_cc, one channel of csdr_amd_wfmrx; the decimator's unprocessed samples and position, the previous sample and the de-emphasis
                             // state stay in the object between passes.  What the four commands write at the default buffer size, without their stale blocks at EOF.
                             // --squelch: squelch_and_smeter_cc in front, inside the object (csdr_amd_wfmrx_create_squelched), as NfmRx's: blocks of the_bufsize
                             // samples, the level protocol and the "%g\n" reports of that command, so `squelch_and_smeter_cc ... | wfm_rx_cc_s16` as one process
    Owned<csdr_amd_wfmrx, csdr_amd_wfmrx_destroy> p; size_t max_n; int sqB = 0, every = 0, fd_out = -1; size_t max_blocks = 0; CtxBuf<float> d_power; std::vector<float> h_power;
    WfmRxStage(csdr_amd_ctx *c, float rate, int points, const float *taps, int nt, float tau, int audio_rate, size_t block) : max_n(block + 1024)
    {
        in_elem = 8; out_elem = 2;
        p.reset(csdr_amd_wfmrx_create(c, 1, rate, points, taps, nt, 1024, tau, audio_rate, max_n));
        if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
    }
    WfmRxStage(csdr_amd_ctx *c, float rate, int points, const float *taps, int nt, float tau, int audio_rate, size_t block, int squelch_block, int use_every_nth,
               int report_every_nth, float level, int out_fd)
        : max_n(block + 1024), sqB(squelch_block), every(report_every_nth), fd_out(out_fd)
    {
        in_elem = 8; out_elem = 2;
        p.reset(csdr_amd_wfmrx_create_squelched(c, 1, rate, points, taps, nt, 1024, tau, audio_rate, max_n, squelch_block, use_every_nth, &level));
        if (!p) { badsyntax(csdr_amd_last_error()); exit(255); }
        max_blocks = max_n / (size_t)squelch_block + 1;
        d_power = ctx_alloc<float>(c, 4 * max_blocks + 64, "malloc"); h_power.resize(max_blocks);
    }
    size_t out_capacity(size_t n) override { return n + 4096 + (size_t)sqB; }
    const char *ctl_format() override { return sqB ? "%g\n" : nullptr; }
    void retune(csdr_amd_ctx *, float level, float) override { MUST(csdr_amd_wfmrx_set_squelch_level(p.get(), 0, level)); fprintf(stderr, "csdr %s: new squelch level is %g\n", g_cmd, level); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t cap, size_t *cons) override
    {
        *cons = n;
        long total = 0;
        for (size_t at = 0; at < n; at += max_n) {                     // (inside `chain` a pass may hand over more than the command's own block)
            const size_t m = std::min(max_n, n - at);
            if (!sqB) {
                const long long na = csdr_amd_wfmrx_process(p.get(), (const csdr_complexf *)i + at, 0, (long long)m, (int16_t *)o + total, nullptr, cap - total);
                MUST(na);
                total += (long)na;
                continue;
            }
            const long long k0 = csdr_amd_wfmrx_squelch_block_index(p.get());
            int nb = 0;
            const long long na = csdr_amd_wfmrx_process_squelched(p.get(), (const csdr_complexf *)i + at, 0, (long long)m, (int16_t *)o + total, nullptr, cap - total, d_power.get(),
                                                                  max_blocks, nullptr, &nb);
            MUST(na);
            total += (long)na;
            bool any = false;
            for (int k = 0; k < nb && !any; k++) any = csdr_amd_squelch_report_due(every, k0 + k) != 0;
            if (any && fd_out >= 0) {
                MUST(csdr_amd_d2h(c, h_power.data(), d_power.get(), 4 * (size_t)nb));
                for (int k = 0; k < nb; k++) if (csdr_amd_squelch_report_due(every, k0 + k)) {
                    char line[101]; const int len = snprintf(line, 100, "%g\n", h_power[k]);
                    (void)!write(fd_out, line, (size_t)len);             // non-blocking: a full fifo drops the line (csdr.c:2211-2228)
                }
            }
        }
        return total;
    }
};

struct DecimatingShift : Stage {   // csdr.c:851-875: one libcsdr call per the_bufsize samples, status carried between calls
    int dec, bufsize; float dsa[3]; void *d_dsa, *d_status;
    DecimatingShift(csdr_amd_ctx *c, float rate, int decimation, int the_bufsize) : dec(decimation), bufsize(the_bufsize)
    {
        in_elem = 8; out_elem = 8; granule = the_bufsize; flush_partial = true;
        csdr_amd_shift_addition_init(rate * (float)decimation, dsa);        // decimating_shift_addition_init libcsdr_gpl.c:126-129
        d_dsa = csdr_amd_malloc(c, 12); d_status = csdr_amd_malloc(c, 12);
        MUST(csdr_amd_h2d(c, d_dsa, dsa, 12)); MUST(csdr_amd_memset(c, d_status, 0, 12));
    }
    size_t out_capacity(size_t n) override { return n / dec + n / bufsize + 16; }
    int next_bufsize(int b) override { return b / dec; }             // csdr.c:861
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        long total = 0;
        for (size_t at = 0; at < n; at += bufsize) {
            const int m = (int)((n - at < (size_t)bufsize) ? n - at : bufsize);
            MUST(csdr_amd_decimating_shift_addition_cc(c, (const csdr_complexf *)i + at, (csdr_complexf *)o + total, 1, m, m, m, d_dsa, dec, d_status));
            int st[3]; MUST(csdr_amd_d2h(c, st, d_status, 12));
            total += st[2];
        }
        return total;
    }
};


// ------------------------------------------------------------------ f2 commands (csdr.c:634-672, 927-983, 1088-1112, 1338-1375, 1569-1661)
struct CfToF : Stage {   // amdemod_cf / amdemod_estimator_cf / realpart_cf / logpower_cf
    int op; float p0;
    CfToF(int o, float a) : op(o), p0(a) { in_elem = 8; out_elem = 4; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        const csdr_complexf *x = (const csdr_complexf *)i; float *y = (float *)o;
        switch (op) {
            case 0: MUST(csdr_amd_amdemod_cf(c, x, y, n)); break;
            case 1: MUST(csdr_amd_amdemod_estimator_cf(c, x, y, n, 0.f, 0.f)); break;            // csdr.c:1108
            case 2: MUST(csdr_amd_realpart_cf(c, x, y, n)); break;
            default: MUST(csdr_amd_logpower_cf(c, x, y, n, p0)); break;
        }
        return (long)n;
    }
};
struct Gain : Stage {    // csdr.c:658-672
    float g; Gain(float gg) : g(gg) { granule = 4; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_gain_ff(c, (const float *)i, (float *)o, n, g)); return (long)n; }
};
struct FmdemodAtan : Stage {   // csdr.c:962-977
    float *d_last;
    FmdemodAtan(csdr_amd_ctx *c) { in_elem = 8; out_elem = 4; d_last = (float *)csdr_amd_malloc(c, 4); MUST(csdr_amd_memset(c, d_last, 0, 4)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_fmdemod_atan_cf(c, (const csdr_complexf *)i, (float *)o, 1, n, n, n, d_last)); return (long)n; }
};
// ------------------------------------------------------------------ transmit-side modulators (csdr.c:2084-2172)
struct TxFlat : Stage {        // dsb_fc / add_dcoffset_cc / fixed_amplitude_cc / convert_f_samplerf
    int op; float p0; unsigned wait;
    TxFlat(int o, float a, unsigned w) : op(o), p0(a), wait(w) { in_elem = o == 0 || o == 3 ? 4 : 8; out_elem = o == 3 ? 16 : 8; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        switch (op) {
            case 0: MUST(csdr_amd_dsb_fc(c, (const float *)i, (csdr_complexf *)o, n, p0)); break;
            case 1: MUST(csdr_amd_add_dcoffset_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, n)); break;
            case 2: MUST(csdr_amd_fixed_amplitude_cc(c, (const csdr_complexf *)i, (csdr_complexf *)o, n, p0)); break;
            default: MUST(csdr_amd_convert_f_samplerf(c, (const float *)i, o, n, wait)); break;
        }
        return (long)n;
    }
};
struct Fmmod : Stage {         // csdr.c:2142-2154: last_phase carried from read to read
    float *d_phase;
    Fmmod(csdr_amd_ctx *c) { in_elem = 4; out_elem = 8; d_phase = (float *)csdr_amd_malloc(c, 4); MUST(csdr_amd_memset(c, d_phase, 0, 4)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_fmmod_fc(c, (const float *)i, (csdr_complexf *)o, 1, n, n, n, d_phase)); return (long)n; }
};
struct DcBlock : Stage {       // csdr.c:927-939 (a = 0 selects 0.999)
    float *d_state;
    DcBlock(csdr_amd_ctx *c) { d_state = (float *)csdr_amd_malloc(c, 8); MUST(csdr_amd_memset(c, d_state, 0, 8)); }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_dcblock_ff(c, (const float *)i, (float *)o, 1, n, n, n, 0.f, d_state)); return (long)n; }
};
struct FastDcBlock : Stage {   // csdr.c:941-960
    int block; float *d_last;
    FastDcBlock(csdr_amd_ctx *c, int b) : block(b) { granule = b; flush_partial = false; d_last = (float *)csdr_amd_malloc(c, 4); MUST(csdr_amd_memset(c, d_last, 0, 4)); }
    int next_bufsize(int) override { return block; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nb = (int)(n / block); *cons = (size_t)nb * block;
        if (nb) MUST(csdr_amd_fastdcblock_ff(c, (const float *)i, (float *)o, 1, nb, block, n, n, d_last));
        return (long)nb * block;
    }
};
struct Agc : Stage {           // csdr.c:1338-1375: one agc_ff call per the_bufsize samples
    short hang, wait; float ref, attack, decay, maxg, alpha; int bufsize; float *d_gain;
    Agc(csdr_amd_ctx *c, int the_bufsize) : bufsize(the_bufsize)
    {
        granule = the_bufsize;
        d_gain = (float *)csdr_amd_malloc(c, 4); const float one = 1.0f; MUST(csdr_amd_h2d(c, d_gain, &one, 4));
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_agc_ff(c, (const float *)i, (float *)o, 1, n, bufsize, n, n, ref, attack, decay, maxg, hang, wait, alpha, d_gain)); return (long)n; }
};
struct FftCc : Stage {         // csdr.c:1569-1641 (binary output; --octave text mode is not offered)
    csdr_amd_fftcc *f; int fft, every;
    FftCc(csdr_amd_ctx *c, int fft_size, int every_n, int window, size_t block) : fft(fft_size), every(every_n)
    {
        in_elem = 8; out_elem = 8; granule = every_n; flush_partial = false;
        f = csdr_amd_fftcc_create(c, fft_size, every_n, window, (int)(block / every_n + 2)); if (!f) die("fftcc_create");
    }
    size_t out_capacity(size_t n) override { return (n / every + 1) * (size_t)fft; }
    int next_bufsize(int) override { return fft; }                   // csdr.c:1596
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { size_t used = 0; int nf = csdr_amd_fftcc_process(f, (const csdr_complexf *)i, n, (csdr_complexf *)o, &used); MUST(nf); *cons = used; return (long)nf * fft; }
};
struct FftFc : Stage {         // csdr.c:3414-3498 (binary output): M complex bins per spectrum of 2M floats; the sliding buffer and the skip stay in the object
    csdr_amd_fftfc *f; int fft, every; size_t chunk;
    FftFc(csdr_amd_ctx *c, int fft_out_size, int every_n, int window, size_t block) : fft(fft_out_size), every(every_n)
    {
        in_elem = 4; out_elem = 8;
        chunk = block + 64;
        if (chunk > (size_t)32768 * every_n) chunk = (size_t)32768 * every_n;      // (the object frames at most 65535 spectra per call)
        f = csdr_amd_fftfc_create(c, fft_out_size, every_n, window, chunk); if (!f) die("fftfc_create");
    }
    size_t out_capacity(size_t n) override { return (n / every + 2) * (size_t)fft; }
    int next_bufsize(int) override { return fft; }                   // csdr.c:3447
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        long nf = 0;
        for (size_t at = 0; at < n; at += chunk) {
            const int k = csdr_amd_fftfc_process(f, (const float *)i + at, n - at < chunk ? n - at : chunk, (csdr_complexf *)o + (size_t)nf * fft); MUST(k);
            nf += k;
        }
        return nf * fft;
    }
};
struct OneSide : Stage {       // csdr.c:1717-1734
    int fft;
    OneSide(int f) : fft(f) { granule = f; flush_partial = false; }
    int next_bufsize(int) override { return fft; }                   // csdr.c:1723
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nr = (int)(n / fft); *cons = (size_t)nr * fft;
        if (nr) MUST(csdr_amd_fft_one_side_ff(c, (const float *)i, (float *)o, nr, fft));
        return (long)nr * (fft / 2);
    }
};


// ------------------------------------------------------------------ f3 commands (csdr.c:1745-1768, 1891-1919)
struct AdpcmEnc : Stage {
    int *d_state;
    AdpcmEnc(csdr_amd_ctx *c) { in_elem = 2; out_elem = 1; granule = 2; flush_partial = false; d_state = (int *)csdr_amd_malloc(c, 8); MUST(csdr_amd_memset(c, d_state, 0, 8)); }
    int next_bufsize(int b) override { return b / 2; }               // csdr.c:1893
    size_t out_capacity(size_t n) override { return n / 2 + 16; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { n &= ~(size_t)1; *cons = n; MUST(csdr_amd_encode_ima_adpcm_i16_u8(c, (const int16_t *)i, (uint8_t *)o, 1, n, n, n / 2, d_state)); return (long)(n / 2); }
};
struct AdpcmDec : Stage {
    int *d_state;
    AdpcmDec(csdr_amd_ctx *c) { in_elem = 1; out_elem = 2; d_state = (int *)csdr_amd_malloc(c, 8); MUST(csdr_amd_memset(c, d_state, 0, 8)); }
    int next_bufsize(int b) override { return b * 2; }               // csdr.c:1910
    size_t out_capacity(size_t n) override { return 2 * n + 16; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    { *cons = n; MUST(csdr_amd_decode_ima_adpcm_u8_i16(c, (const uint8_t *)i, (int16_t *)o, 1, n, n, 2 * n, d_state)); return (long)(2 * n); }
};
struct CompressFft : Stage {
    int fft;
    CompressFft(int f) : fft(f) { in_elem = 4; out_elem = 1; granule = f; flush_partial = false; }
    int next_bufsize(int) override { return fft + 10; }              // csdr.c:1752
    size_t out_capacity(size_t n) override { return (n / fft + 1) * (size_t)((fft + 10) / 2) + 16; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nb = (int)(n / fft); *cons = (size_t)nb * fft;
        if (nb) MUST(csdr_amd_compress_fft_adpcm_f_u8(c, (const float *)i, (uint8_t *)o, nb, fft));
        return (long)nb * ((fft + 10) / 2);
    }
};

// ------------------------------------------------------------------ the waterfall (csdr.c:1663-1714; waterfall.hip)
struct LogAvgPower : Stage {   // csdr.c:1663-1695: avgnumber spectra in, one row out; reads no preamble and sends none
    int fft, avg; float add_db;
    LogAvgPower(int f, int a, float db) : fft(f), avg(a), add_db(db) { in_elem = 8; out_elem = 4; granule = (size_t)f * a; flush_partial = false; }
    int next_bufsize(int) override { return -1; }
    size_t out_capacity(size_t n) override { return (n / granule + 1) * (size_t)fft; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nr = (int)(n / granule); *cons = (size_t)nr * granule;
        if (nr) MUST(csdr_amd_logaveragepower_cf(c, (const csdr_complexf *)i, (float *)o, nr, fft, avg, add_db));
        return (long)nr * fft;
    }
};
struct ExchangeSides : Stage {   // csdr.c:1697-1714
    int fft;
    ExchangeSides(int f) : fft(f) { granule = f; flush_partial = false; }
    int next_bufsize(int) override { return fft; }                   // csdr.c:1705
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        const int nr = (int)(n / fft); *cons = (size_t)nr * fft;
        if (nr) MUST(csdr_amd_fft_exchange_sides_ff(c, (const float *)i, (float *)o, nr, fft));
        return (long)nr * fft;
    }
};
// `[convert_u8_f |] fft_cc N E [window] | logaveragepower_cf A N AVG | fft_exchange_sides_ff N [| compress_fft_adpcm_f_u8 N]` as ONE command (extension):
//   csdr waterfall_u8 | waterfall_cc <fft_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm>
// and `[convert_s16_f |] fft_fc M E [window] | logaveragepower_cf A M AVG [| compress_fft_adpcm_f_u8 M]` on a real stream (one-sided rows, M = output bins):
//   csdr waterfall_ff | waterfall_s16 <fft_out_size> <every_n> <window> <add_db> <avgnumber> <db|adpcm>
struct WaterfallStage : Stage {
    csdr_amd_waterfall *w; int fft, every, avg; bool adpcm;
    WaterfallStage(csdr_amd_ctx *c, int in_format, int f, int e, int window, float add_db, int a, bool ad, size_t block) : fft(f), every(e), avg(a), adpcm(ad)
    {
        in_elem = in_format == CSDR_AMD_WF_IN_CF32 ? 8 : in_format == CSDR_AMD_WF_IN_F32 ? 4 : 2; out_elem = ad ? 1 : 4;
        w = csdr_amd_waterfall_create(c, f, e, window, a, add_db, in_format, ad ? CSDR_AMD_WF_OUT_ADPCM : CSDR_AMD_WF_OUT_DB, 1, block + 64);
        if (!w) die("waterfall_create");
    }
    size_t row_elems() const { return adpcm ? (size_t)(fft + 10) / 2 : (size_t)fft; }
    size_t out_capacity(size_t n) override { return ((n + fft) / every / avg + 2) * row_elems(); }
    int next_bufsize(int) override { return adpcm ? fft + 10 : fft; }  // what the last stage of the pattern sends (csdr.c:1752, 1705)
    long process(csdr_amd_ctx *, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;                                                    // overlap, skip and partial row stay in the object
        int rows = 0;
        MUST(csdr_amd_waterfall_process(w, i, n, n, o, 0, &rows));
        return (long)((size_t)rows * row_elems());
    }
};

// ------------------------------------------------------------------ noise sources, AWGN channel, timing variance (csdr.c:3035-3146)
// --seed S, or eight bytes read once from /dev/urandom
unsigned long long noise_seed_arg(int argc, char **argv, int from)
{
    for (int k = from; k + 1 < argc; k++) if (!strcmp(argv[k], "--seed")) return strtoull(argv[k + 1], nullptr, 0);
    unsigned long long seed = 0;
    FILE *f = fopen("/dev/urandom", "r");
    if (!f || fread(&seed, sizeof seed, 1, f) != 1) { badsyntax("failed to read a seed from /dev/urandom"); exit(255); }
    fclose(f);
    return seed;
}

struct Awgn : Stage {   // awgn_cc csdr.c:3035-3091.  Without --awgnfile the noise is the seeded stream of one csdr_amd_noise channel, added in the generating kernel:
                       // the output does not depend on how the passes cut the stream.  With it, the file's whole blocks of the_bufsize samples cycle as in the
                       // reference (a short read rewinds: the partial tail is never used): stream sample k takes noise sample k mod (whole blocks x the_bufsize).
                       // --snrshow: one "SNR = %f dB" line per the_bufsize samples, as the reference prints (file mode: from the powers of the unscaled rows and the gains).
    Owned<csdr_amd_noise, csdr_amd_noise_destroy> p; CtxBuf<csdr_complexf> d_noise; CtxBuf<float> d_g, d_snr; size_t period = 0, at = 0; int B; bool snrshow; float a_signal, g_noise;
    Awgn(csdr_amd_ctx *c, float snr_db, const char *awgnfile, bool show, unsigned long long seed, int the_bufsize) : B(the_bufsize), snrshow(show)
    {
        in_elem = 8; out_elem = 8;
        if (show) granule = (size_t)the_bufsize;
        csdr_amd_awgn_gains(snr_db, &a_signal, &g_noise);
        const float a_noise = g_noise / 0.707f;
        fprintf(stderr, "csdr %s: a_signal = %f, a_noise = %f\n", g_cmd, a_signal, a_noise);
        d_snr = ctx_alloc<float>(c, 64, "malloc");
        if (!awgnfile) {
            p.reset(csdr_amd_noise_create(c, 1, CSDR_AMD_NOISE_GAUSSIAN, seed, nullptr)); if (!p) die("noise_create");
            MUST(csdr_amd_noise_set_snr_db(p.get(), 0, snr_db));
            return;
        }
        FILE *f = fopen(awgnfile, "r");
        if (!f) { badsyntax("failed to open the --awgnfile"); exit(255); }
        std::vector<csdr_complexf> h;
        std::vector<csdr_complexf> blk((size_t)the_bufsize);
        while (fread(blk.data(), sizeof(csdr_complexf), blk.size(), f) == blk.size()) h.insert(h.end(), blk.begin(), blk.end());
        fclose(f);
        if (h.empty()) { badsyntax("the --awgnfile holds less than one buffer of samples"); exit(255); }
        period = h.size();
        d_noise = ctx_alloc<csdr_complexf>(c, 8 * period, "malloc");
        MUST(csdr_amd_h2d(c, d_noise.get(), h.data(), 8 * period));
        d_g = ctx_alloc<float>(c, 64, "malloc");
        const float gains[2] = {a_signal, g_noise};
        MUST(csdr_amd_h2d(c, d_g.get(), gains, sizeof gains));
    }
    float fetch(csdr_amd_ctx *c) { float v = 0; MUST(csdr_amd_d2h(c, &v, d_snr.get(), 4)); return v; }
    // one run of m samples whose noise is contiguous
    void piece(csdr_amd_ctx *c, const csdr_complexf *x, csdr_complexf *y, size_t m, bool with_snr)
    {
        if (p) {
            MUST(csdr_amd_noise_awgn_cc(p.get(), x, (long long)m, m, y, m, with_snr ? d_snr.get() : nullptr));
            if (with_snr) fprintf(stderr, "csdr %s: SNR = %f dB\n", g_cmd, fetch(c));
            return;
        }
        if (with_snr) {
            MUST(csdr_amd_total_logpower_cf(c, x, 1, (long long)m, m, d_snr.get()));
            const float ps = fetch(c) + 20 * log10f(a_signal);
            MUST(csdr_amd_total_logpower_cf(c, d_noise.get() + at, 1, (long long)m, m, d_snr.get()));
            fprintf(stderr, "csdr %s: SNR = %f dB\n", g_cmd, ps - (fetch(c) + 20 * log10f(g_noise)));
        }
        MUST(csdr_amd_awgn_cc(c, x, d_noise.get() + at, y, 1, (long long)m, m, m, m, d_g.get(), d_g.get() + 1));
        at = (at + m) % period;
    }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        const csdr_complexf *x = (const csdr_complexf *)i; csdr_complexf *y = (csdr_complexf *)o;
        for (size_t done = 0; done < n;) {
            size_t m = n - done;
            if (snrshow) m = std::min(m, (size_t)B);
            if (!p) m = std::min(m, period - at);
            piece(c, x + done, y + done, m, snrshow);
            done += m;
        }
        return (long)n;
    }
};

struct TimingVariance : Stage {   // normalized_timing_variance_u32_f csdr.c:3121-3146: one float per the_bufsize indexes (a partial last buffer gives one of its own)
    int B, sps, offset; CtxBuf<float> d_out; std::vector<float> h;
    TimingVariance(int the_bufsize, int s, int off) : B(the_bufsize), sps(s), offset(off) { in_elem = 4; out_elem = 4; granule = (size_t)the_bufsize; }
    size_t out_capacity(size_t n) override { return n / B + 16; }
    long process(csdr_amd_ctx *c, const void *i, size_t n, void *o, size_t, size_t *cons) override
    {
        *cons = n;
        const size_t rows = n / B, rest = n % B;
        if (rows) MUST(csdr_amd_normalized_timing_variance_u32_f(c, (const unsigned *)i, (size_t)B, B, nullptr, (int)rows, sps, offset, (float *)o));
        if (rest) MUST(csdr_amd_normalized_timing_variance_u32_f(c, (const unsigned *)i + rows * B, rest, (int)rest, nullptr, 1, sps, offset, (float *)o + rows));
        const size_t k = rows + (rest ? 1 : 0);
        h.resize(k);
        if (k) MUST(csdr_amd_d2h(c, h.data(), o, 4 * k));
        for (float v : h) fprintf(stderr, "csdr %s: normalized variance = %f\n", g_cmd, v);
        return (long)k;
    }
};

// `csdr uniform_noise_f [--seed S]` / `csdr gaussian_noise_c [--seed S]` (csdr.c:3093-3119): sources, they write until the reader goes away
int run_noise_source(csdr_amd_ctx *c, int argc, char **argv, bool gaussian)
{
    const unsigned long long seed = noise_seed_arg(argc, argv, 2);
    Owned<csdr_amd_noise, csdr_amd_noise_destroy> p(csdr_amd_noise_create(c, 1, gaussian ? CSDR_AMD_NOISE_GAUSSIAN : CSDR_AMD_NOISE_UNIFORM, seed, nullptr));
    if (!p) die("noise_create");
    const size_t elem = gaussian ? 8 : 4, n = std::max((size_t)unitround(g_dynamic ? 1024 : g_fixed), (size_t)65536);
    const auto d = ctx_alloc<char>(c, elem * n, "malloc");
    std::vector<char> h(elem * n);
    for (;;) {
        MUST(csdr_amd_noise_generate(p.get(), d.get(), (long long)n, n));
        MUST(csdr_amd_d2h(c, h.data(), d.get(), h.size()));
        if (fwrite(h.data(), 1, h.size(), stdout) != h.size() || fflush(stdout)) return 0;
    }
}

// Build the operator for one command line.  `block` = the largest input this stage will be handed in one call.
// ctl: opened when the command line carries --fifo/--fd (single-command mode only).  Returns nullptr after printing why.
// the BPSK31 commands: stage index, parameters into *pr, *extra = 1 / 2 for --output_error / --output_indexes; -1 (message given) on bad syntax
int parse_psk31(int argc, char **argv, csdr_amd_psk31_params *pr, int *extra)
{
    const std::string cmd = argv[1];
    if (cmd == "simple_agc_cc") {                                                   // csdr.c:2902-2921
        if (argc <= 2) { badsyntax("need required parameter (rate)"); return -1; }
        sscanf(argv[2], "%f", &pr->rate);
        if (pr->rate <= 0) { badsyntax("rate should be > 0"); return -1; }
        pr->reference = 1.f; if (argc > 3) sscanf(argv[3], "%f", &pr->reference);
        if (pr->reference <= 0) { badsyntax("reference should be > 0"); return -1; }
        pr->max_gain = 65535.f; if (argc > 4) sscanf(argv[4], "%f", &pr->max_gain);
        if (pr->max_gain <= 0) { badsyntax("max_gain should be > 0"); return -1; }
        return CSDR_AMD_PSK31_AGC;
    }
    if (cmd == "timing_recovery_cc") {                                              // csdr.c:2573-2618
        if (argc <= 2) { badsyntax("need required parameter (algorithm)"); return -1; }
        pr->algorithm = !strcmp(argv[2], "EARLYLATE") ? 1 : 0;                      // timing_recovery_get_algorithm_from_string: anything else is GARDNER
        if (argc <= 3) { badsyntax("need required parameter (decimation factor)"); return -1; }
        int d = 0; sscanf(argv[3], "%d", &d);
        if (d <= 4 || (d & 3)) { badsyntax("decimation factor should be a positive integer divisible by 4"); return -1; }
        pr->decimation = d;
        pr->loop_gain = 0.5f; if (argc > 4) sscanf(argv[4], "%f", &pr->loop_gain);
        pr->max_error = 2.f; if (argc > 5) sscanf(argv[5], "%f", &pr->max_error);
        const int add_q = argc >= 7 && !strcmp(argv[6], "--add_q");
        pr->use_q = add_q;
        if (argc >= 7 + add_q && !strncmp(argv[6 + add_q], "--octave", 8)) { badsyntax("--octave / --octave_save (debug plots) are not supported"); return -1; }
        *extra = 0;
        if (argc >= 7 + add_q && !strcmp(argv[6 + add_q], "--output_error")) *extra = 1;
        if (argc >= 7 + add_q && !strcmp(argv[6 + add_q], "--output_indexes")) *extra = 2;
        return CSDR_AMD_PSK31_TIMING;
    }
    if (cmd == "dbpsk_decoder_c_u8") return CSDR_AMD_PSK31_DBPSK;
    if (cmd == "psk31_varicode_decoder_u8_u8") return CSDR_AMD_PSK31_VARICODE;
    return -2;
}

// the BPSK31 transmit commands: stage index, n_psk / interpolation into their arguments; -1 (message given) on bad syntax, -2: not one of them
int parse_psk31tx(int argc, char **argv, int *n_psk, int *interpolation)
{
    const std::string cmd = argv[1];
    if (cmd == "psk31_varicode_encoder_u8_u8") return CSDR_AMD_PSK31TX_VARICODE;
    if (cmd == "differential_encoder_u8_u8") return CSDR_AMD_PSK31TX_DIFF;
    if (cmd == "psk_modulator_u8_c") {                                              // csdr.c:2684-2689
        if (argc <= 2) { badsyntax("need required parameter (n_psk)"); return -1; }
        int v = 0; sscanf(argv[2], "%d", &v);
        if (v <= 0 || v > 256) { badsyntax("n_psk should be between 1 and 256"); return -1; }
        *n_psk = v;
        return CSDR_AMD_PSK31TX_MOD;
    }
    if (cmd == "psk31_interpolate_sine_cc") {                                       // csdr.c:2727-2732
        if (argc <= 2) { badsyntax("need required parameter (interpolation)"); return -1; }
        int v = 0; sscanf(argv[2], "%d", &v);
        if (v <= 0) { badsyntax("interpolation should be >0"); return -1; }
        *interpolation = v;
        return CSDR_AMD_PSK31TX_SHAPE;
    }
    return -2;
}

// the RTTY commands: stage index, parameters into *pr; -1 (message given) on bad syntax.  B: the serial decoder's window, as the reference's
// getbufsize() gives it with bigbufs (csdr.c:332): the fixed big buffer, or the preamble's size in dynamic mode
int parse_rtty(int argc, char **argv, csdr_amd_rtty_params *pr, int B)
{
    const std::string cmd = argv[1];
    if (cmd == "bfsk_demod_cf") {                                                   // csdr.c:3271-3284
        if (argc <= 2) { badsyntax("required parameter <frequency_shift> is missing."); return -1; }
        sscanf(argv[2], "%f", &pr->spacing);
        if (argc <= 3) { badsyntax("required parameter <filter_length> is missing."); return -1; }
        sscanf(argv[3], "%d", &pr->filter_length);
        if (pr->filter_length < 1) { badsyntax("filter_length should be at least 1"); return -1; }
        return CSDR_AMD_RTTY_BFSK;
    }
    if (cmd == "serial_line_decoder_f_u8") {                                        // csdr.c:2490-2507
        if (argc <= 2) { badsyntax("need required parameter (samples_per_bits)"); return -1; }
        sscanf(argv[2], "%f", &pr->samples_per_bits);
        if (pr->samples_per_bits < 1) { badsyntax("samples_per_bits should be at least 1."); return -1; }
        if (pr->samples_per_bits < 5) fprintf(stderr, "%s: warning: this algorithm does not work well if samples_per_bits is too low. It should be at least 5.\n", argv[1]);
        pr->databits = 8; if (argc > 3) sscanf(argv[3], "%d", &pr->databits);
        if (pr->databits > 8 || pr->databits < 1) { badsyntax("databits should be between 1 and 8."); return -1; }
        pr->stopbits = 1; if (argc > 4) sscanf(argv[4], "%f", &pr->stopbits);
        if (pr->stopbits < 1) { badsyntax("stopbits should be equal or above 1."); return -1; }
        pr->bit_sampling_width_ratio = 0.4f;
        pr->cli_bufsize = B;
        if ((float)2 + pr->samples_per_bits * ((float)(1 + pr->databits) + pr->stopbits) >= (float)B) {
            badsyntax("a character does not fit in the buffer: serial_line_decoder_f_u8() would get stuck (raise CSDR_FIXED_BUFSIZE)"); return -1;
        }
        return CSDR_AMD_RTTY_SERIAL;
    }
    if (cmd == "rtty_baudot2ascii_u8_u8") return CSDR_AMD_RTTY_BAUDOT;
    return -2;
}

Stage *make_stage(csdr_amd_ctx *c, int argc, char **argv, size_t block, Control *ctl, int the_bufsize)
{
    {
        const int B = g_dynamic ? unitround(the_bufsize) : unitround(g_fixed_big);
        if (!strcmp(argv[1], "rtty_rx")) {                                          // `chain`'s fused RTTY run: argv[2..] are its commands, one per argument
            csdr_amd_rtty_params pr; memset(&pr, 0, sizeof pr); pr.window = the_bufsize;
            int first = -1, last = -1;
            for (int k = 2; k < argc; k++) {
                std::vector<std::string> words = split_chain(argv[k])[0]; std::vector<char *> av = argv_of(words);
                g_cmd = av[1];
                const int st = parse_rtty((int)av.size(), av.data(), &pr, B);
                if (st < 0) return nullptr;
                if (first < 0) first = st;
                last = st;
            }
            g_cmd = argv[1];
            return new Rtty(c, pr, first, last);
        }
        csdr_amd_rtty_params pr; memset(&pr, 0, sizeof pr); pr.window = the_bufsize;
        const char *keep = g_cmd; g_cmd = argv[1];
        const int st = parse_rtty(argc, argv, &pr, B);
        if (st == -1) return nullptr;
        if (st >= 0) return new Rtty(c, pr, st, st);
        g_cmd = keep;
        if (!strcmp(argv[1], "rtty_line_decoder_u8_u8")) return new RttyLine(c);
        if (!strcmp(argv[1], "binary_slicer_f_u8")) return new BinarySlicer();
    }
    if (!strcmp(argv[1], "psk31_rx")) {                                             // `chain`'s fused BPSK31 run: argv[2..] are its commands, one per argument
        csdr_amd_psk31_params pr; memset(&pr, 0, sizeof pr);
        int first = -1, last = -1, extra = 0;
        for (int k = 2; k < argc; k++) {
            std::vector<std::string> words = split_chain(argv[k])[0]; std::vector<char *> av = argv_of(words);
            const int st = parse_psk31((int)av.size(), av.data(), &pr, &extra);
            if (st < 0) return nullptr;
            if (first < 0) first = st;
            last = st;
        }
        return new Psk31(c, pr, first, last, last == CSDR_AMD_PSK31_TIMING ? extra : 0);
    }
    {
        csdr_amd_psk31_params pr; memset(&pr, 0, sizeof pr); int extra = 0;
        const int st = parse_psk31(argc, argv, &pr, &extra);
        if (st == -1) return nullptr;
        if (st >= 0) return new Psk31(c, pr, st, st, extra);
    }
    if (!strcmp(argv[1], "psk31_tx")) {                                             // `chain`'s fused BPSK31 transmit run: argv[2..] are its commands, one per argument
        int n_psk = 2, interpolation = 1, first = -1, last = -1;
        for (int k = 2; k < argc; k++) {
            std::vector<std::string> words = split_chain(argv[k])[0]; std::vector<char *> av = argv_of(words);
            g_cmd = av[1];
            const int st = parse_psk31tx((int)av.size(), av.data(), &n_psk, &interpolation);
            if (st < 0) return nullptr;
            if (first < 0) first = st;
            last = st;
        }
        g_cmd = argv[1];
        return new Psk31Tx(c, n_psk, interpolation, first, last);
    }
    {
        int n_psk = 2, interpolation = 1;
        const char *keep = g_cmd; g_cmd = argv[1];
        const int st = parse_psk31tx(argc, argv, &n_psk, &interpolation);
        if (st == -1) return nullptr;
        if (st >= 0) return new Psk31Tx(c, n_psk, interpolation, st, st);
        if (!strcmp(argv[1], "differential_decoder_u8_u8")) return new DiffDecoder(c);
        if (!strcmp(argv[1], "duplicate_samples_ntimes_u8_u8")) {                   // csdr.c:2704-2712
            int sample_size_bytes = 0, ntimes = 0;
            if (argc <= 2) { badsyntax("need required parameter (sample_size_bytes)"); return nullptr; }
            sscanf(argv[2], "%d", &sample_size_bytes);
            if (sample_size_bytes <= 0) { badsyntax("sample_size_bytes should be >0"); return nullptr; }
            if (argc <= 3) { badsyntax("need required parameter (ntimes)"); return nullptr; }
            sscanf(argv[3], "%d", &ntimes);
            if (ntimes <= 0) { badsyntax("ntimes should be >0"); return nullptr; }
            return new DuplicateSamples(sample_size_bytes, ntimes);
        }
        g_cmd = keep;
    }
    if (!strcmp(argv[1], "pulse_tx")) {                                             // `chain`'s fused pulse-shaping run: argv[2..] are its commands, one per argument
        int n_psk = 2, interpolation = 1, first = CSDR_AMD_PULSETX_SHAPE; std::vector<float> taps;
        for (int k = 2; k < argc; k++) {
            std::vector<std::string> words = split_chain(argv[k])[0]; std::vector<char *> av = argv_of(words);
            g_cmd = av[1];
            if (!strcmp(av[1], "psk_modulator_u8_c")) { int unused = 1; if (parse_psk31tx((int)av.size(), av.data(), &n_psk, &unused) < 0) return nullptr; first = CSDR_AMD_PULSETX_MOD; }
            else if (!strcmp(av[1], "plain_interpolate_cc")) { if (!parse_plain_interpolate((int)av.size(), av.data(), &interpolation)) return nullptr; }
            else if (!parse_pulse_filter((int)av.size(), av.data(), &taps)) return nullptr;
        }
        g_cmd = argv[1];
        if (taps.empty()) { badsyntax("pulse_tx: the run ends with pulse_shaping_filter_cc"); return nullptr; }
        return new PulseTx(c, n_psk, interpolation, taps, first);
    }
    if (!strcmp(argv[1], "pulse_rx")) {                                             // `chain`'s fused receive run: argv[2..] are its commands, one per argument
        std::vector<float> taps; csdr_amd_psk31_params tr; memset(&tr, 0, sizeof tr);
        csdr_amd_pulserx_params pr; memset(&pr, 0, sizeof pr);
        bool realpart = false, sliced = false;
        for (int k = 2; k < argc; k++) {
            std::vector<std::string> words = split_chain(argv[k])[0]; std::vector<char *> av = argv_of(words);
            g_cmd = av[1];
            if (!strcmp(av[1], "pulse_shaping_filter_cc")) { if (!parse_pulse_filter((int)av.size(), av.data(), &taps)) return nullptr; }
            else if (!strcmp(av[1], "timing_recovery_cc")) { int extra = 0; if (parse_psk31((int)av.size(), av.data(), &tr, &extra) < 0) return nullptr; }
            else if (!strcmp(av[1], "realpart_cf")) realpart = true;
            else if (!strcmp(av[1], "gain_ff")) { if (av.size() <= 2) { badsyntax("need required parameter (gain)"); return nullptr; } sscanf(av[2], "%g", &pr.gain); }
            else if (!strcmp(av[1], "generic_slicer_f_u8")) {                       // csdr.c:3221-3225
                if (av.size() <= 2) { badsyntax("required parameter <n_symbols> is missing."); return nullptr; }
                sscanf(av[2], "%d", &pr.n_symbols);
                if (pr.n_symbols < 2 || pr.n_symbols > 256) { badsyntax("n_symbols should be between 2 and 256"); return nullptr; }
                sliced = true;
            }
        }
        g_cmd = argv[1];
        if (taps.empty() || !tr.decimation) { badsyntax("pulse_rx: the run starts with pulse_shaping_filter_cc | timing_recovery_cc"); return nullptr; }
        pr.taps = taps.data(); pr.taps_length = (int)taps.size();
        pr.algorithm = tr.algorithm; pr.decimation = tr.decimation; pr.loop_gain = tr.loop_gain; pr.max_error = tr.max_error; pr.use_q = tr.use_q;
        pr.slice_q = sliced && !realpart;
        return new PulseRx(c, pr, sliced ? CSDR_AMD_PULSERX_SLICE : CSDR_AMD_PULSERX_TIMING);
    }
    if (!strcmp(argv[1], "plain_interpolate_cc")) {
        const char *keep = g_cmd; g_cmd = argv[1];
        int interpolation = 0;
        if (!parse_plain_interpolate(argc, argv, &interpolation)) return nullptr;
        g_cmd = keep;
        return new PlainInterpolate(interpolation);
    }
    if (!strcmp(argv[1], "pulse_shaping_filter_cc")) {
        const char *keep = g_cmd; g_cmd = argv[1];
        std::vector<float> taps;
        if (!parse_pulse_filter(argc, argv, &taps)) return nullptr;
        g_cmd = keep;
        return new PulseFilter(c, taps);
    }
    if (!strcmp(argv[1], "peaks_fir_cc")) {                                         // csdr.c:2975-2995, its checks in its order
        const char *keep = g_cmd; g_cmd = argv[1];
        if (argc <= 2) { badsyntax("need required parameter (taps_length)"); return nullptr; }
        int taps_length = 0; sscanf(argv[2], "%d", &taps_length);
        std::vector<float> rates;
        for (int k = 3; k < argc; k++) { float r = 0; sscanf(argv[k], "%f", &r); rates.push_back(r); }
        if (rates.empty()) { badsyntax("need required parameter (peak_rate) once or multiple times"); return nullptr; }
        if (the_bufsize - taps_length <= 0) { badsyntax("taps_length is below buffer size, decrease taps_length"); return nullptr; }
        if (taps_length < 1) { badsyntax("taps_length should be at least 1"); return nullptr; }
        g_cmd = keep;
        return new PeaksFir(c, taps_length, rates);
    }
    if (!strcmp(argv[1], "generic_slicer_f_u8")) {                                  // csdr.c:3221-3225
        const char *keep = g_cmd; g_cmd = argv[1];
        int n_symbols = 0;
        if (argc <= 2) { badsyntax("required parameter <n_symbols> is missing."); return nullptr; }
        sscanf(argv[2], "%d", &n_symbols);
        if (n_symbols < 2 || n_symbols > 256) { badsyntax("n_symbols should be between 2 and 256"); return nullptr; }
        g_cmd = keep;
        return new GenericSlicer(n_symbols);
    }
    if (!strcmp(argv[1], "pattern_search_u8_u8")) {                                 // csdr.c:3532-3546, its checks in its order; [--mismatch <m>] in front is ours
        const char *keep = g_cmd; g_cmd = argv[1];
        int a = 2, values_after = 0, mismatch = 0;
        if (argc > 3 && !strcmp(argv[2], "--mismatch")) { sscanf(argv[3], "%d", &mismatch); a = 4; }
        if (argc <= a) { badsyntax("need required parameter (values_after)"); return nullptr; }
        sscanf(argv[a], "%d", &values_after);
        if (argc <= a + 1) { badsyntax("need required parameter (pattern_values × N)"); return nullptr; }
        std::vector<unsigned> pattern(argc - a - 1, 0u);
        for (size_t k = 0; k < pattern.size(); k++) sscanf(argv[a + 1 + k], "%u", &pattern[k]);
        fprintf(stderr, "csdr %s: pattern values: ", g_cmd);
        for (unsigned v : pattern) fprintf(stderr, "%x ", v);
        fprintf(stderr, "\n");
        for (unsigned v : pattern) if (v > 255) { badsyntax("a pattern value above 255 cannot match a byte (the reference would output nothing)"); return nullptr; }
        Stage *s = new FrameSync(c, pattern, values_after, mismatch);
        g_cmd = keep;
        return s;
    }
    if (!strcmp(argv[1], "pack_bits_1to8_u8_u8")) return new PackBits(true);
    if (!strcmp(argv[1], "pack_bits_8to1_u8_u8")) return new PackBits(false);
    g_cmd = argv[1];
    const std::string cmd = argv[1];
    const bool has_ctl = ctl && ctl->open_from(argc, argv);
    if (cmd == "squelch_and_smeter_cc") {                                           // csdr.c:2192-2218, its checks in its order
        float level = 0, unused;
        if (!has_ctl) { badsyntax("need required parameter (--fifo <fifo>)"); return nullptr; }
        ctl->wait_first("%g\n", &level, &unused);
        fprintf(stderr, "csdr %s: initial squelch level is %g\n", g_cmd, level);
        if (argc <= 5 || strcmp(argv[4], "--outfifo")) { badsyntax("need required parameter (--outfifo <fifo>)"); return nullptr; }
        const int fd2 = open(argv[5], O_WRONLY);
        if (fd2 == -1) { badsyntax("error while opening --outfifo"); return nullptr; }
        fcntl(fd2, F_SETFL, fcntl(fd2, F_GETFL, 0) | O_NONBLOCK);
        if (argc <= 6) { badsyntax("need required parameter (use_every_nth)"); return nullptr; }
        int decimation = 0, report_every_nth = 0;
        sscanf(argv[6], "%d", &decimation);
        if (decimation <= 0) { badsyntax("use_every_nth <= 0 is invalid"); return nullptr; }
        if (argc <= 7) { badsyntax("need required parameter (report_every_nth)"); return nullptr; }
        sscanf(argv[7], "%d", &report_every_nth);
        if (report_every_nth <= 0) { badsyntax("report_every_nth <= 0 is invalid"); return nullptr; }
        return new Squelch(c, g_dynamic ? the_bufsize : unitround(g_fixed), decimation, report_every_nth, level, fd2, block);   // without the preamble protocol every reference process has its default buffer
    }
    if (cmd == "bpsk_costas_loop_cc") {                                             // csdr.c:2834-2873, its checks in its order
        float bw = 0, damping = 0;
        if (argc <= 2) { badsyntax("need required parameter (loop_bandwidth)"); return nullptr; }
        sscanf(argv[2], "%f", &bw);
        if (argc <= 3) { badsyntax("need required parameter (damping_factor)"); return nullptr; }
        sscanf(argv[3], "%f", &damping);
        // (the reference tests argv[5] for the long spelling and passes a mode its init never stores: here argv[4] alone selects the mode)
        const int dd = argc > 4 && (!strcmp(argv[4], "--dd") || !strcmp(argv[4], "--decision_directed"));
        if (dd) fprintf(stderr, "csdr %s: decision directed mode\n", g_cmd);
        const char *opt = argc > 4 + dd ? argv[4 + dd] : "";
        const int which = !strcmp(opt, "--output_error") ? Carrier::ERROR : !strcmp(opt, "--output_dphase") ? Carrier::DPHASE : !strcmp(opt, "--output_nco") ? Carrier::NCO
                        : !strcmp(opt, "--output_combined") ? Carrier::COMBINED : Carrier::OUT;
        csdr_amd_carrier_params pr; csdr_amd_costas_params(bw, damping, dd, &pr);
        fprintf(stderr, "csdr %s: alpha = %f, beta = %f\n", g_cmd, pr.alpha, pr.beta);
        FILE *f[3] = {nullptr, nullptr, nullptr};
        if (which == Carrier::COMBINED) {
            if (!(argc > 4 + dd + 3)) { badsyntax("need required parameters after --output_combined: <error_file> <dphase_file> <nco_file>"); return nullptr; }
            for (int k = 0; k < 3; k++) { f[k] = fopen(argv[4 + dd + 1 + k], "w"); if (!f[k]) { badsyntax("error while opening an --output_combined file"); return nullptr; } }
        }
        return new Carrier(c, pr, which, f[0], f[1], f[2]);
    }
    if (cmd == "pll_cc") {                                                          // csdr.c:2532-2557: the NCO is the output
        if (argc <= 2) { badsyntax("need required parameter (pll_type)"); return nullptr; }
        int type = 0; sscanf(argv[2], "%d", &type);
        csdr_amd_carrier_params pr;
        if (type == 1) {
            float alpha = 0.01f; if (argc > 3) sscanf(argv[3], "%f", &alpha);
            csdr_amd_pll_params_p(alpha, &pr);
        } else if (type == 2) {
            float bandwidth = 0.01f, ko = 10, kd = 0.1f, damping = 0.707f;
            if (argc > 3) sscanf(argv[3], "%f", &bandwidth);
            if (argc > 4) sscanf(argv[4], "%f", &damping);
            if (argc > 5) sscanf(argv[5], "%f", &ko);
            if (argc > 6) sscanf(argv[6], "%f", &kd);
            csdr_amd_pll_params_pi(bandwidth, ko, kd, damping, &pr);
            fprintf(stderr, "csdr %s: bw=%f damping=%f ko=%f kd=%f alpha=%f beta=%f\n", g_cmd, bandwidth, damping, ko, kd, pr.alpha, pr.beta);
        } else { badsyntax("invalid pll_type. Valid values are:\n\t1: PLL_P_CONTROLLER\n\t2: PLL_PI_CONTROLLER"); return nullptr; }
        return new Carrier(c, pr, Carrier::NCO);
    }
    if (cmd == "awgn_cc") {                                                         // csdr.c:3035-3049: <snr_db> [--awgnfile F] [--snrshow]; [--seed S] is ours
        if (argc <= 2) { badsyntax("required parameter <snr_db> is missing."); return nullptr; }
        float snr_db = 0; sscanf(argv[2], "%f", &snr_db);
        const char *file = nullptr; bool show = false;
        for (int k = 3; k < argc; k++) {
            if (!strcmp(argv[k], "--awgnfile") && k + 1 < argc) file = argv[++k];
            else if (!strcmp(argv[k], "--snrshow")) show = true;
            else if (!strcmp(argv[k], "--seed") && k + 1 < argc) k++;
        }
        return new Awgn(c, snr_db, file, show, file ? 0 : noise_seed_arg(argc, argv, 3), unitround(the_bufsize));
    }
    if (cmd == "normalized_timing_variance_u32_f") {                                // csdr.c:3121-3132 (--debug, its stderr trace, is not offered)
        if (argc <= 2) { badsyntax("required parameter <samples_per_symbol> is missing."); return nullptr; }
        if (argc <= 3) { badsyntax("required parameter <initial_sample_offset> is missing."); return nullptr; }
        int sps = 0, off = 0; sscanf(argv[2], "%d", &sps); sscanf(argv[3], "%d", &off);
        if (sps < 1) { badsyntax("samples_per_symbol should be at least 1"); return nullptr; }
        return new TimingVariance(unitround(the_bufsize), sps, off);
    }
    if (cmd == "convert_u8_f") return new Convert(0, 1, 4);
    if (cmd == "convert_f_u8") return new Convert(1, 4, 1);
    if (cmd == "convert_s8_f") return new Convert(2, 1, 4);
    if (cmd == "convert_f_s8") return new Convert(3, 4, 1);
    if (cmd == "convert_f_s16" || cmd == "convert_f_i16") return new Convert(4, 4, 2);
    if (cmd == "convert_s16_f" || cmd == "convert_i16_f") return new Convert(5, 2, 4);
    if (cmd == "convert_f_s24") { Convert *cv = new Convert(6, 4, 3); cv->bigendian = argc > 2 && !strcmp(argv[2], "--bigendian"); cv->granule = 4; return cv; }
    if (cmd == "convert_s24_f") { Convert *cv = new Convert(7, 3, 4); cv->bigendian = argc > 2 && !strcmp(argv[2], "--bigendian"); cv->granule = 4; return cv; }
    if (cmd == "shift_math_cc" || cmd == "shift_addition_cc" || cmd == "shift_table_cc" || cmd == "shift_addfast_cc" || cmd == "shift_unroll_cc" || cmd == "shift_addition_fc") {
        float rate = 0;
        const bool ctl_cmd = cmd == "shift_addition_cc" || cmd == "shift_addition_fc" || cmd == "shift_addfast_cc" || cmd == "shift_unroll_cc";
        if (has_ctl && ctl_cmd) { float d; ctl->wait_first("%g\n", &rate, &d); }
        else { if (argc <= 2) { badsyntax("need required parameter (rate)"); return nullptr; } sscanf(argv[2], "%g", &rate); }
        int variant = CSDR_SHIFT_ADDITION, aux = 0;
        if (cmd == "shift_math_cc") variant = CSDR_SHIFT_MATH;
        else if (cmd == "shift_table_cc") { variant = CSDR_SHIFT_TABLE; aux = 65536; if (argc > 3) sscanf(argv[3], "%d", &aux); }       // csdr.c:731
        else if (cmd == "shift_addfast_cc") variant = CSDR_SHIFT_ADDFAST;
        else if (cmd == "shift_unroll_cc") { variant = CSDR_SHIFT_UNROLL; aux = 1024; }                                                  // csdr.c:821
        Shift *sh = new Shift(variant, rate, aux);
        if (cmd == "shift_addition_fc") { sh->real_in = true; sh->in_elem = 4; }
        return sh;
    }
    if (cmd == "decimating_shift_addition_cc") {
        if (argc <= 2) { badsyntax("need required parameter (rate)"); return nullptr; }
        float rate; int dec = 1; sscanf(argv[2], "%g", &rate); if (argc > 3) sscanf(argv[3], "%d", &dec);
        if (dec < 1) { badsyntax("decimation must be >= 1"); return nullptr; }
        return new DecimatingShift(c, rate, dec, the_bufsize);
    }
    if (cmd == "fir_decimate_cc") {
        if (argc <= 2) { badsyntax("need required parameter (decimation factor)"); return nullptr; }
        int factor = 0;
        if (sscanf(argv[2], "%d", &factor) != 1 || factor < 1) { badsyntax("decimation factor must be an integer >= 1"); return nullptr; }
        float tbw = 0.05f; if (argc >= 4) sscanf(argv[3], "%g", &tbw);
        if (!(tbw > 0)) { badsyntax("transition_bw must be positive"); return nullptr; }
        return new FirDecimate(c, factor, tbw, window_arg(argc, argv, 4, "fir_decimate_cc"));
    }
    if (cmd == "fmdemod_quadri_cf" || cmd == "fmdemod_quadri_novect_cf") return new Fmdemod(c);
    if (cmd == "limit_ff") { float m = 1.0f; if (argc >= 3) sscanf(argv[2], "%g", &m); return new Limit(m); }
    if (cmd == "deemphasis_wfm_ff") {
        if (argc <= 3) { badsyntax("need required parameters (sample rate, tau)"); return nullptr; }
        int rate; float tau; sscanf(argv[2], "%d", &rate); sscanf(argv[3], "%g", &tau);
        fprintf(stderr, "csdr deemphasis_wfm_ff: tau = %g, sample_rate = %d\n", tau, rate);
        return new DeemphWfm(c, rate, tau);
    }
    if (cmd == "deemphasis_nfm_ff") { if (argc <= 2) { badsyntax("need required parameter (sample rate)"); return nullptr; } int rate; sscanf(argv[2], "%d", &rate); return new DeemphNfm(c, rate, g_dynamic ? the_bufsize : unitround(g_fixed)); }   // without the preamble protocol every reference process has its default buffer
    if (cmd == "fastagc_ff") { int b = 1024; float ref = 1.0f; if (argc >= 3) sscanf(argv[2], "%d", &b); if (argc >= 4) sscanf(argv[3], "%g", &ref); if (b <= 0) { badsyntax("block size must be positive"); return nullptr; } return new FastAgc(c, b, ref); }
    if (cmd == "fractional_decimator_ff") {
        if (argc <= 2) { badsyntax("need required parameters (rate)"); return nullptr; }
        float rate; sscanf(argv[2], "%g", &rate);
        if (rate == 1) return new Copy();
        int points = 12; if (argc >= 4) sscanf(argv[3], "%d", &points);
        if (points & 1) { badsyntax("num_poly_points should be even"); return nullptr; }
        if (points < 2) { badsyntax("num_poly_points should be >= 2"); return nullptr; }
        std::vector<float> taps;
        if (argc >= 5 && !strcmp(argv[4], "--prefilter")) {                          // csdr.c:1481-1486, 1499-1507: only --prefilter enables it
            const float tbw = 0.03f;
            const int nt = csdr_amd_firdes_filter_len(tbw); taps.resize(nt);
            csdr_amd_firdes_lowpass_f(taps.data(), nt, 0.5f / (rate - tbw), CSDR_WINDOW_HAMMING);
        }
        return new FracDec(rate, points, taps.empty() ? nullptr : taps.data(), (int)taps.size(), g_dynamic ? the_bufsize : unitround(g_fixed));
    }
    if (cmd == "rational_resampler_ff" || cmd == "suboptimal_rational_resampler_ff") {   // csdr.c:1409-1430
        if (argc <= 3) { badsyntax("need required parameters (interpolation, decimation)"); return nullptr; }
        int I = 0, D = 0; sscanf(argv[2], "%d", &I); sscanf(argv[3], "%d", &D);
        if (I < 1 || D < 1) { badsyntax("interpolation and decimation must be integers >= 1"); return nullptr; }
        if (I == 1 && D == 1) return new Copy();
        float tbw = 0.05f; if (argc >= 5) sscanf(argv[4], "%g", &tbw);
        if (!(tbw > 0)) { badsyntax("transition_bw must be positive"); return nullptr; }
        const int window = window_arg(argc, argv, 5, g_cmd);
        if (cmd[0] == 's') fprintf(stderr, "csdr %s: note: suboptimal rational resampler chosen.\n", g_cmd);
        return new Resample(c, I, D, tbw, window, g_dynamic ? the_bufsize : unitround(g_fixed));
    }
    if (cmd == "fir_interpolate_cc") {   // csdr.c:1179-1201
        if (argc <= 2) { badsyntax("need required parameter (interpolation factor)"); return nullptr; }
        int factor = 0; sscanf(argv[2], "%d", &factor);
        if (factor < 1) { badsyntax("interpolation factor must be an integer >= 1"); return nullptr; }
        float tbw = 0.05f; if (argc >= 4) sscanf(argv[3], "%g", &tbw);
        if (!(tbw > 0 && tbw < 1)) { badsyntax("transition_bw must be in (0, 1)"); return nullptr; }
        const int window = window_arg(argc, argv, 4, g_cmd);
        int big = g_fixed_big;                                       // csdr.c:1198: the big buffer doubles until it holds two filters
        while (big < 2 * csdr_amd_firdes_filter_len(tbw)) big *= 2;
        return new Interp(c, factor, tbw, window, g_dynamic ? the_bufsize : unitround(big));
    }
    if (cmd == "bandpass_fir_fft_cc") {
        float lo = 0, hi = 0, tbw = 0;
        if (has_ctl) { ctl->wait_first("%g %g\n", &lo, &hi); if (argc <= 4) { badsyntax("need more required parameters (transition_bw)"); return nullptr; } }
        else { if (argc <= 4) { badsyntax("need required parameters (low_cut, high_cut, transition_bw)"); return nullptr; } sscanf(argv[2], "%g", &lo); sscanf(argv[3], "%g", &hi); }
        sscanf(argv[4], "%g", &tbw);
        return new Bandpass(c, lo, hi, tbw, argc >= 6 ? window_from(argv[5]) : CSDR_WINDOW_HAMMING, block);
    }
    if (cmd == "fastddc_fwd_cc") {
        if (argc <= 2) { badsyntax("need required parameter (decimation)"); return nullptr; }
        int D; sscanf(argv[2], "%d", &D); float tbw = 0.05f; if (argc > 3) sscanf(argv[3], "%g", &tbw);
        return new DdcFwd(c, D, tbw, block);
    }
    if (cmd == "fastddc_inv_cc") {
        float shift = 0; int plus = 0;
        if (has_ctl) { float d; ctl->wait_first("%g\n", &shift, &d); plus = 1; }
        else { if (argc <= 2) { badsyntax("need required parameter (rate)"); return nullptr; } sscanf(argv[2], "%g", &shift); }
        if (argc <= 3 + plus) { badsyntax("need required parameter (decimation)"); return nullptr; }
        int D; sscanf(argv[3 + plus], "%d", &D);
        float tbw = 0.05f; if (argc > 4 + plus) sscanf(argv[4 + plus], "%g", &tbw);
        return new DdcInv(c, shift, D, tbw, argc > 5 + plus ? window_from(argv[5 + plus]) : CSDR_WINDOW_HAMMING, block);
    }
    if (cmd == "amdemod_cf") return new CfToF(0, 0);
    if (cmd == "amdemod_estimator_cf") return new CfToF(1, 0);
    if (cmd == "realpart_cf") return new CfToF(2, 0);
    if (cmd == "logpower_cf") { float add_db = 0; if (argc >= 3) sscanf(argv[2], "%g", &add_db); return new CfToF(3, add_db); }
    if (cmd == "gain_ff") { if (argc <= 2) { badsyntax("need required parameter (gain)"); return nullptr; } float g; sscanf(argv[2], "%g", &g); return new Gain(g); }
    if (cmd == "fmdemod_atan_cf") return new FmdemodAtan(c);
    if (cmd == "dsb_fc") { float q = 0; if (argc >= 3) sscanf(argv[2], "%g", &q); return new TxFlat(0, q, 0); }
    if (cmd == "add_dcoffset_cc") return new TxFlat(1, 0, 0);
    if (cmd == "fixed_amplitude_cc") {
        if (argc <= 2) { badsyntax("need required parameter (new_amplitude)"); return nullptr; }
        float a = 0; sscanf(argv[2], "%g", &a); return new TxFlat(2, a, 0);
    }
    if (cmd == "convert_f_samplerf") {
        if (argc <= 2) { badsyntax("need required parameter (wait_for_this_sample)"); return nullptr; }
        unsigned w = 0; sscanf(argv[2], "%u", &w); return new TxFlat(3, 0, w);
    }
    if (cmd == "fmmod_fc") return new Fmmod(c);
    if (cmd == "dcblock_ff") return new DcBlock(c);
    if (cmd == "fastdcblock_ff") { int b = 1024; if (argc >= 3) sscanf(argv[2], "%d", &b); if (b <= 0) { badsyntax("block size must be positive"); return nullptr; } return new FastDcBlock(c, b); }
    if (cmd == "agc_ff") {   // defaults csdr.c:1343-1361
        Agc *a = new Agc(c, the_bufsize);
        a->hang = 200; a->ref = 0.2f; a->attack = 0.01f; a->decay = 0.0001f; a->maxg = 65536; a->wait = 0; a->alpha = 0.999f;
        if (argc >= 3) sscanf(argv[2], "%hd", &a->hang);
        if (argc >= 4) sscanf(argv[3], "%g", &a->ref);
        if (argc >= 5) sscanf(argv[4], "%g", &a->attack);
        if (argc >= 6) sscanf(argv[5], "%g", &a->decay);
        if (argc >= 7) sscanf(argv[6], "%g", &a->maxg);
        if (argc >= 8) sscanf(argv[7], "%hd", &a->wait);
        if (argc >= 9) sscanf(argv[8], "%g", &a->alpha);
        return a;
    }
    if (cmd == "fft_cc") {
        if (argc <= 3) { badsyntax("need required parameters (fft_size, out_of_every_n_samples)"); return nullptr; }
        int fft, every; sscanf(argv[2], "%d", &fft); sscanf(argv[3], "%d", &every);
        if (csdr_amd_log2n(fft) == -1) { badsyntax("fft_size should be power of 2"); return nullptr; }
        if (every <= 0) { badsyntax("out_of_every_n_samples must be positive"); return nullptr; }
        if (argc >= 6 && !strcmp(argv[5], "--octave")) { badsyntax("--octave text output is not offered by the MI355X back end"); return nullptr; }
        return new FftCc(c, fft, every, argc >= 5 ? window_from(argv[4]) : CSDR_WINDOW_HAMMING, block);
    }
    if (cmd == "encode_ima_adpcm_i16_u8" || cmd == "encode_ima_adpcm_s16_u8") return new AdpcmEnc(c);
    if (cmd == "decode_ima_adpcm_u8_i16" || cmd == "decode_ima_adpcm_u8_s16") return new AdpcmDec(c);
    if (cmd == "compress_fft_adpcm_f_u8") {
        if (argc <= 2) { badsyntax("need required parameters (fft_size)"); return nullptr; }
        int fft; sscanf(argv[2], "%d", &fft);
        if (fft <= 0 || (fft & 1)) { badsyntax("fft_size must be positive and even"); return nullptr; }
        return new CompressFft(fft);
    }
    if (cmd == "logaveragepower_cf") {
        if (argc <= 4) { badsyntax("need required parameters (add_db, fft_size, avgnumber)"); return nullptr; }
        float add_db = 0; int fft = 0, avg = 0;
        sscanf(argv[2], "%g", &add_db); sscanf(argv[3], "%d", &fft); sscanf(argv[4], "%d", &avg);
        if (csdr_amd_log2n(fft) < 1 || avg <= 0) { badsyntax("fft_size must be a power of two >= 2 and avgnumber positive"); return nullptr; }
        return new LogAvgPower(fft, avg, add_db);
    }
    if (cmd == "fft_exchange_sides_ff") {
        if (argc <= 2) { badsyntax("need required parameters (fft_size)"); return nullptr; }
        int fft = 0; sscanf(argv[2], "%d", &fft);
        if (csdr_amd_log2n(fft) < 1) { badsyntax("fft_size must be a power of two >= 2"); return nullptr; }
        return new ExchangeSides(fft);
    }
    if (cmd == "fft_fc") {
        if (argc <= 3) { badsyntax("need required parameters (fft_out_size, out_of_every_n_samples)"); return nullptr; }
        int fft = 0, every = 0; sscanf(argv[2], "%d", &fft); sscanf(argv[3], "%d", &every);
        if (csdr_amd_log2n(fft) < 1) { badsyntax("fft_out_size should be power of 2 (>= 2 on the MI355X back end)"); return nullptr; }
        if (every <= 0) { badsyntax("out_of_every_n_samples must be positive"); return nullptr; }
        if (argc >= 6 && !strcmp(argv[5], "--octave")) { badsyntax("--octave text output is not offered by the MI355X back end"); return nullptr; }
        return new FftFc(c, fft, every, argc >= 5 ? window_from(argv[4]) : CSDR_WINDOW_HAMMING, block);
    }
    if (cmd == "fft_one_side_ff") {
        if (argc <= 2) { badsyntax("need required parameters (fft_size)"); return nullptr; }
        int fft = 0; sscanf(argv[2], "%d", &fft);
        if (fft < 2 || (fft & 1)) { badsyntax("fft_size must be even and >= 2"); return nullptr; }
        return new OneSide(fft);
    }
    if (cmd == "waterfall_u8" || cmd == "waterfall_cc" || cmd == "waterfall_ff" || cmd == "waterfall_s16") {
        if (argc <= 7) { badsyntax("need required parameters (fft_size, every_n, window, add_db, avgnumber, db|adpcm)"); return nullptr; }
        int fft = 0, every = 0, avg = 0; float add_db = 0;
        sscanf(argv[2], "%d", &fft); sscanf(argv[3], "%d", &every); sscanf(argv[5], "%g", &add_db); sscanf(argv[6], "%d", &avg);
        if (csdr_amd_log2n(fft) < 1 || every <= 0 || avg <= 0) { badsyntax("fft_size must be a power of two >= 2, every_n and avgnumber positive"); return nullptr; }
        const int in_format = cmd == "waterfall_u8" ? CSDR_AMD_WF_IN_U8 : cmd == "waterfall_cc" ? CSDR_AMD_WF_IN_CF32 : cmd == "waterfall_ff" ? CSDR_AMD_WF_IN_F32 : CSDR_AMD_WF_IN_S16;
        return new WaterfallStage(c, in_format, fft, every, window_from(argv[4]), add_db, avg, !strcmp(argv[7], "adpcm"), block);
    }
    if (cmd == "nfm_rx_cc_s16") {                                       // [audio_rate] [--squelch --fifo <ctl> --outfifo <path> <use_every_nth> <report_every_nth>]
        int rate = 48000, a = 2;
        if (argc > 2 && strcmp(argv[2], "--squelch")) { if (sscanf(argv[2], "%d", &rate) != 1) { badsyntax("the audio rate must be a number"); return nullptr; } a = 3; }
        if (argc <= a) return new NfmRx(c, rate, block);
        if (strcmp(argv[a], "--squelch")) { badsyntax("the argument behind the audio rate is --squelch"); return nullptr; }
        // squelch_and_smeter_cc's arguments and checks in its order (csdr.c:2192-2218), behind --squelch
        char **sv = argv + (a - 1); const int sc = argc - (a - 1);       // sv[2] is what follows --squelch
        float level = 0, unused;
        if (!ctl || !ctl->open_from(sc, sv)) { badsyntax("need required parameter (--fifo <fifo>)"); return nullptr; }
        ctl->wait_first("%g\n", &level, &unused);
        fprintf(stderr, "csdr %s: initial squelch level is %g\n", g_cmd, level);
        if (sc <= 5 || strcmp(sv[4], "--outfifo")) { badsyntax("need required parameter (--outfifo <fifo>)"); return nullptr; }
        const int fd2 = open(sv[5], O_WRONLY);
        if (fd2 == -1) { badsyntax("error while opening --outfifo"); return nullptr; }
        fcntl(fd2, F_SETFL, fcntl(fd2, F_GETFL, 0) | O_NONBLOCK);
        if (sc <= 6) { badsyntax("need required parameter (use_every_nth)"); return nullptr; }
        int decimation = 0, report_every_nth = 0;
        sscanf(sv[6], "%d", &decimation);
        if (decimation <= 0) { badsyntax("use_every_nth <= 0 is invalid"); return nullptr; }
        if (sc <= 7) { badsyntax("need required parameter (report_every_nth)"); return nullptr; }
        sscanf(sv[7], "%d", &report_every_nth);
        if (report_every_nth <= 0) { badsyntax("report_every_nth <= 0 is invalid"); return nullptr; }
        return new NfmRx(c, rate, block, g_dynamic ? the_bufsize : unitround(g_fixed), decimation, report_every_nth, level, fd2);   // the squelch command's own block
    }
    if (cmd == "wfm_rx_cc_s16") {                                       // <rate> [audio_rate [tau [num_poly_points [--prefilter [transition_bw [window]]]]]]
                                                                        // [--squelch --fifo <ctl> --outfifo <path> <use_every_nth> <report_every_nth>] behind any prefix of them
        int sq_at = 0;                                                  // argv index of --squelch: it ends the optional arguments
        for (int k = 3; k < argc && !sq_at; k++) if (!strcmp(argv[k], "--squelch")) sq_at = k;
        const int all_argc = argc;
        if (sq_at) argc = sq_at;
        if (argc <= 2) { badsyntax("need required parameters (rate)   usage: wfm_rx_cc_s16 <rate> [audio_rate [tau [num_poly_points [--prefilter [transition_bw [window]]]]]]"); return nullptr; }
        float rate = 0, tau = 50e-6f, tbw = 0.03f; int audio_rate = 48000, points = 12;
        if (sscanf(argv[2], "%g", &rate) != 1) { badsyntax("the rate must be a number"); return nullptr; }
        if (argc > 3 && sscanf(argv[3], "%d", &audio_rate) != 1) { badsyntax("the audio rate must be a number"); return nullptr; }
        if (argc > 4 && sscanf(argv[4], "%g", &tau) != 1) { badsyntax("tau must be a number"); return nullptr; }
        if (argc > 5 && sscanf(argv[5], "%d", &points) != 1) { badsyntax("num_poly_points must be a number"); return nullptr; }
        std::vector<float> taps;
        if (argc > 6) {
            if (strcmp(argv[6], "--prefilter")) { badsyntax("the argument behind num_poly_points is --prefilter"); return nullptr; }
            if (argc > 7 && (sscanf(argv[7], "%g", &tbw) != 1 || !(tbw > 0))) { badsyntax("transition_bw must be a positive number"); return nullptr; }
            const int nt = csdr_amd_firdes_filter_len(tbw); taps.resize(nt);                        // csdr.c:1506-1509
            csdr_amd_firdes_lowpass_f(taps.data(), nt, 0.5f / (rate - tbw), window_arg(argc, argv, 8, g_cmd));
        }
        if (!sq_at) return new WfmRxStage(c, rate, points, taps.empty() ? nullptr : taps.data(), (int)taps.size(), tau, audio_rate, block);
        // squelch_and_smeter_cc's arguments and checks in its order (csdr.c:2192-2218), behind --squelch, as nfm_rx_cc_s16's
        char **sv = argv + (sq_at - 1); const int sc = all_argc - (sq_at - 1);       // sv[2] is what follows --squelch
        float level = 0, unused;
        if (!ctl || !ctl->open_from(sc, sv)) { badsyntax("need required parameter (--fifo <fifo>)"); return nullptr; }
        ctl->wait_first("%g\n", &level, &unused);
        fprintf(stderr, "csdr %s: initial squelch level is %g\n", g_cmd, level);
        if (sc <= 5 || strcmp(sv[4], "--outfifo")) { badsyntax("need required parameter (--outfifo <fifo>)"); return nullptr; }
        const int fd2 = open(sv[5], O_WRONLY);
        if (fd2 == -1) { badsyntax("error while opening --outfifo"); return nullptr; }
        fcntl(fd2, F_SETFL, fcntl(fd2, F_GETFL, 0) | O_NONBLOCK);
        if (sc <= 6) { badsyntax("need required parameter (use_every_nth)"); return nullptr; }
        int decimation = 0, report_every_nth = 0;
        sscanf(sv[6], "%d", &decimation);
        if (decimation <= 0) { badsyntax("use_every_nth <= 0 is invalid"); return nullptr; }
        if (sc <= 7) { badsyntax("need required parameter (report_every_nth)"); return nullptr; }
        sscanf(sv[7], "%d", &report_every_nth);
        if (report_every_nth <= 0) { badsyntax("report_every_nth <= 0 is invalid"); return nullptr; }
        return new WfmRxStage(c, rate, points, taps.empty() ? nullptr : taps.data(), (int)taps.size(), tau, audio_rate, block, g_dynamic ? the_bufsize : unitround(g_fixed),
                              decimation, report_every_nth, level, fd2);               // the squelch command's own block
    }
    // the fused commands: `--fifo <path>` / `--fd <n>` stand where the shift rate stands, as in shift_addition_cc (csdr.c:881-893); the first rate is waited for
    if (cmd == "ddc_u8_cc" || cmd == "nfm_chain_u8_s16" || cmd == "wfm_chain_u8_s16") {
        float shift = 0;
        int a = 3;                                                   // argv index of the first argument behind the rate
        if (has_ctl) { float d; ctl->wait_first("%g\n", &shift, &d); a = 4; }
        else if (argc > 2) sscanf(argv[2], "%g", &shift);
        else if (cmd == "ddc_u8_cc") { badsyntax("need required parameters (shift rate, decimation factor)"); return nullptr; }
        if (cmd == "ddc_u8_cc") {
            if (argc <= a) { badsyntax("need required parameters (shift rate, decimation factor)"); return nullptr; }
            float tbw = 0.05f; int factor = 0; sscanf(argv[a], "%d", &factor);
            if (factor < 1) { badsyntax("decimation factor must be >= 1"); return nullptr; }
            if (argc > a + 1) sscanf(argv[a + 1], "%g", &tbw);
            const int window = argc > a + 2 ? window_from(argv[a + 2]) : CSDR_WINDOW_HAMMING;
            return new DdcFront(c, shift, factor, tbw, window, block, has_ctl);
        }
        if (cmd == "nfm_chain_u8_s16") {
            float tbw = 0.005f; int factor = 50;
            if (argc > a) sscanf(argv[a], "%d", &factor);
            if (argc > a + 1) sscanf(argv[a + 1], "%g", &tbw);
            return new NfmChain(c, shift, factor, tbw, block, has_ctl);
        }
        { const char *rs = getenv("CSDR_AMD_RESIDENT"); if (rs && atoi(rs)) return new WfmRingStage(c, shift, has_ctl); }
        return new WfmChain(c, shift, block, has_ctl);
    }
    fprintf(stderr, "csdr: function \"%s\" is not part of the MI355X hot path (see --help)\n", argv[1]);
    return nullptr;
}
