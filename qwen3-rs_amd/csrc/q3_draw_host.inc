// q3_draw_host.inc -- the draw site, stated once on the host (included by q3_engine.hip in front of q3_engine; no kernels here).
// A draw site is where Sampler::sample runs on the device (q3_sampler.h, q3_topk.h): sampler states and scratch for `cols` columns
// of logits.  There are four: the single-stream engine's (q3_engine::draw, 1 column), the batched decode's (BatchCtx::draw_decode,
// max_streams columns), the column passes' and the verify pass's (BatchCtx::draw_cols, kSpecMax columns) and the temporary one of
// the operator entry points.  Their sizes (draw_sizes), their memory (DrawSite::alloc), their kernel arguments (draw_args) and
// their launches (draw_launches) are written here and nowhere else.

namespace {

// What a vocabulary of n entries needs per column: blen terms per lane block of k_sample, n2 keys per half of the sort scratch
// (the next power of two >= n), `scratch` floats of probs and of sp.
struct DrawSizes {
    int blen;
    size_t n2, scratch;
};
DrawSizes draw_sizes(int n) {
    DrawSizes z{4 * ((n + 4095) / 4096), 1, 0};
    while (z.n2 < (size_t)n) z.n2 <<= 1;
    z.scratch = (size_t)kSampThreads * z.blen;
    return z;
}

// How a site's launches address it.  Engine: one column, the chip-wide passes of the pipelined draw, the developer timeline.
// Decode and Columns: a workgroup per column, strides between the columns; Columns commits nothing itself (the turn / commit
// kernels read the drawn tokens from the column states).  Operator: one column, k_sample alone.
enum class DrawForm { Engine, Decode, Columns, Operator };

// The memory of a site: an allocation group (q3_mem.h), and the arguments its launches carry.  Move-only like its members; false
// until alloc() has succeeded.
struct DrawSite {
    DevMem<SamplerState> ss;             // [cols] sampler states
    DevMem<float> probs, sp;             // [cols][scratch]
    DevMem<unsigned long long> keys;     // [cols][2 * n2]
    DevMem<float> hist;                  // the engine's site: mass histogram and per-workgroup candidate counts of the pipelined draw
    DevMem<int> counts;
    int n = 0;                           // vocabulary size
    SampleArgs args{}, tail{};           // draw_args: what its launches carry; tail: the second k_sample of the pipelined draw
    SampleArgs pen{};                    // draw_args_pen: args over the penalised rows of section 2p (the column site alone; logits null: not set)
    explicit operator bool() const { return ss != nullptr; }

    // One group, committed whole: a failed allocation leaves the site with none of it, and the next call starts over.
    // chip_passes: also hist / counts.
    int alloc(int vocab, int cols, bool chip_passes) {
        const DrawSizes z = draw_sizes(vocab);
        const size_t c = (size_t)cols;
        DevMem<SamplerState> ss_; DevMem<float> probs_, sp_, hist_; DevMem<unsigned long long> keys_; DevMem<int> counts_;
        int rc;
        if ((rc = ss_.alloc(c)) || (rc = probs_.alloc(z.scratch * c)) || (rc = sp_.alloc(z.scratch * c)) || (rc = keys_.alloc(2 * z.n2 * c)) ||
            (chip_passes && ((rc = hist_.alloc(kSampHistBins)) || (rc = counts_.alloc(kSampGrid)))))
            return rc;
        ss = std::move(ss_); probs = std::move(probs_); sp = std::move(sp_);
        keys = std::move(keys_); hist = std::move(hist_); counts = std::move(counts_);
        n = vocab;
        return Q3_OK;
    }
};

// The one place a SampleArgs is filled: site `s` drawing over `logits` and the states `st`, drawn tokens to out_tokens (a window of
// out_cap per column; 0 closes it).  stamps: the Engine form's developer timeline.
void draw_args(DrawSite& s, DrawForm form, const float* logits, State* st, int32_t* out_tokens, int out_cap,
               unsigned long long* stamps = nullptr) {
    const DrawSizes z = draw_sizes(s.n);
    const bool strided = form == DrawForm::Decode || form == DrawForm::Columns;
    SampleArgs a{};
    a.logits = logits;
    a.n = s.n;
    a.blen = z.blen;
    a.probs = s.probs;
    a.keys = s.keys;
    a.keys2_off = (long long)z.n2;
    a.sp = s.sp;
    a.ss = s.ss;
    a.st = st;
    a.out_tokens = out_tokens;
    a.out_cap = out_cap;
    if (strided) {
        a.sb_logits = s.n;
        a.sb_scratch = (long long)z.scratch;
        a.sb_keys = 2 * (long long)z.n2;
    }
    a.pre_exp = form == DrawForm::Columns ? 1 : form == DrawForm::Operator ? 0 : dev_knob("Q3_SAMPLER_PRE_EXP", 1);
    if (form == DrawForm::Engine) {
        a.phase = (a.pre_exp && dev_knob("Q3_SAMPLER_PIPELINE", 1)) ? 1 : 0;
        a.hist = s.hist;
        a.counts = s.counts;
        a.stamps = stamps;
    }
    s.args = s.tail = a;
    s.tail.phase = 2;
}

// The one place the arguments of a draw over PENALISED rows are stated (section 2p): what draw_args left in s.args, with the rows of
// q3_penalty.h's buffer -- [columns][n], the classifier's stride -- in place of the classifier's output.  Whoever makes the second of
// the two (the column site, the penalty state) calls it; both exist before a plan that draws under penalties is built.
void draw_args_pen(DrawSite& s, const float* pen_logits) {
    s.pen = s.args;
    s.pen.logits = pen_logits;
    s.pen.sb_logits = s.n;
}
// the arguments a site's launches carry: over the classifier's rows, or (pen) over the penalised ones
const SampleArgs& draw_site_args(const DrawSite& s, bool pen) { return pen ? s.pen : s.args; }

// the top-k launches' view of a draw: its logits, states and outputs are the site's SampleArgs', k and the slices' lists are given
TopkArgs topk_args(const SampleArgs& s, int* k, unsigned long long* part_keys) {
    TopkArgs t{};
    t.logits = s.logits;
    t.sb_logits = s.sb_logits;
    t.n = s.n;
    t.parts = topk_parts();
    t.k = k;
    t.part_keys = part_keys;
    t.ss = s.ss;
    t.st = s.st;
    t.out_tokens = s.out_tokens;
    t.out_cap = s.out_cap;
    return t;
}

// The launches of one draw of the first `cols` columns of a site, stated once.  topk null: Sampler::sample as it is -- the
// element-wise exp pass on exp_parts workgroups per column where pre_exp is set, then a workgroup per column; pipelined
// (phase 1, one column): that workgroup keeps the order-sensitive parts (exact sum; sort + exact walks) and the element-wise
// passes over the vocabulary in between run on the whole chip.  topk: the selection over the slices of every column, then one
// wave per column (q3_topk.h).  put(kernel, grid, block, lds_bytes, args) appends one launch to a plan or enqueues it at once.
template <class Put>
int draw_launches(const DrawSite& site, int cols, unsigned exp_parts, const TopkArgs* topk, Put&& put, bool pen = false) {
    const SampleArgs& a = draw_site_args(site, pen);
    int rc;
    const dim3 per_col((unsigned)cols);
    if (topk) {
        if ((rc = put(k_topk_part, dim3((unsigned)topk->parts, (unsigned)cols), dim3(256), 0, *topk))) return rc;
        return put(k_topk_draw, per_col, dim3(64), 0, *topk);
    }
    if (a.pre_exp && (rc = put(k_sample_exp, dim3(exp_parts, (unsigned)cols), dim3(256), 0, a))) return rc;
    if ((rc = put(k_sample, per_col, dim3(kSampThreads), 4 * kSegFloats, a)) || a.phase != 1) return rc;
    if ((rc = put(k_sample_norm_hist, dim3(kSampGrid), dim3(256), 0, a)) || (rc = put(k_sample_count, dim3(kSampGrid), dim3(256), 0, a)) ||
        (rc = put(k_sample_scatter, dim3(kSampGrid), dim3(256), 0, a)))
        return rc;
    return put(k_sample, per_col, dim3(kSampThreads), 4 * kSegFloats, site.tail);
}
constexpr unsigned kDrawExpParts = 64;   // exp_parts of the batched sites (the engine's site: a workgroup per CU)

}  // namespace
