// spal_csr_tune.hip -- setup-time measurements on a planned CSR handle: the autotune (kernel form, placement of the
// 16-bit columns) and spal_csr_alloc_vectors with the placement walk.  Products are launched through csr_launch only.
#include "spal_internal.hpp"

namespace spal {

// Times the applicable variants of the planned kernel on the caller's vectors
// and keeps the fastest (all variants compute identical results).  Setup-time
// work: it synchronises `stream`.
//  1. form: one super-tile per workgroup, or the walking form -- the sliding-window kernel when the plan has
//     it (bands), else the persistent form -- each with plain or non-temporal y stores;
//  1b. where the plan built row records (csr_rowrec.hpp) and the sliding kernel was kept: records against col16;
//  1c. where the plan packed the values (csr_valpack.hpp) and the record form was kept: packed values against the values;
//  2. placement of the column array the kept form streams (the records, or the 16-bit columns) relative to the values (two streams out of one class of region of the device's
//     memory disturb each other): the columns are tried in up to `place_tries` blocks of 1 GiB taken one
//     after the other from the device's memory; the fastest place is kept.
template <typename T>
static int csr_autotune(spal_csr_t a, const T *x_dev, T *y_dev, void *stream, int iters) {
    if (!a) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_autotune: handle is NULL");
    if (a->elem_size != (int)sizeof(T))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_autotune: handle holds %s values",
                    a->elem_size == 8 ? "f64" : "f32");
    if (!x_dev || !y_dev) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_autotune: null vector");
    if (!a->parts.empty()) {   // row blocks: each tunes its own plan on its rows of y
        for (size_t b = 0; b < a->parts.size(); ++b)
            SPAL_TRY(csr_autotune<T>(a->parts[b], x_dev, y_dev + a->part_row0[b], stream, iters));
        return SPAL_OK;
    }
    if (iters < 1) iters = 1;
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    SPAL_TRY(csr_ensure_plan(a, nullptr, false));
    if (a->bw_on) return SPAL_OK;   // (nothing to tune: one kernel, its geometry fixed by the windows)
    if (a->split_short) return csr_autotune<T>(a->split_short, x_dev, y_dev, stream, iters);   // (the short part's kernels; y is scratch here)
    std::lock_guard<std::mutex> lock(a->mu);
    CsrPlan &p = a->plan;
    for (float &t : a->tuned_us) t = 0.f;
    a->place_us[0] = a->place_us[1] = 0.f;
    a->place_tried = 0;
    if (a->nnz == 0 || p.kernel != 2 || p.tiles_per_wave != 4) return SPAL_OK;  // nothing to choose from
    hipStream_t st = (hipStream_t)stream;
    SetupTimer timer;
    int rc = SPAL_OK;
    auto timed = [&](int n, float *ms_per_launch) {   // n launches of the current configuration (after 3 untimed)
        if (rc != SPAL_OK) return;
        float ms = 0.f;
        rc = timer.run(st, 3, n, [&] { return csr_launch(a, x_dev, y_dev, st); }, &ms, "spal_csr_autotune");
        *ms_per_launch = ms / (float)n;
    };
    // ---- 0. columns anywhere: the column-blocked kernel against the stream kernels (results are bit-identical)
    a->cblock_us[0] = a->cblock_us[1] = 0.f;
    {   // (under the lock a first product on another thread takes for the same build, csr_launch)
        std::lock_guard<std::mutex> lock(a->mu_cb);
        if (p.cblock_pending) {
            (void)cblock_plan(a, false);
            __atomic_store_n(&p.cblock_pending, 0, __ATOMIC_RELEASE);
        }
    }
    if (p.cblock) {
        float ms[2] = {0.f, 0.f};
        for (int round = 0; round < 2 && rc == SPAL_OK; ++round)
            for (int on = 0; on < 2 && rc == SPAL_OK; ++on) { p.cblock_on = on; timed(std::max(3, iters / 3), &ms[on]); }
        if (rc == SPAL_OK) {
            a->cblock_us[0] = ms[0] * 1e3f; a->cblock_us[1] = ms[1] * 1e3f;
            p.cblock_on = ms[1] <= ms[0] ? 1 : 0;
        }
        if (p.cblock_on) return rc;   // nothing of the stream kernels' forms to choose
    }
    // ---- 1. the form.  candidate c: bit 0 = walking form (sliding kernel / persistent), bit 1 = non-temporal y stores
    const bool walking_is_slide = p.slide != 0;
    const int planned = ((walking_is_slide ? p.slide_on : p.persistent) ? 1 : 0) | (p.nt_store ? 2 : 0);   // what the plan chose by structure
    int best = planned;
    float best_ms = 1e30f, planned_ms = 1e30f;
    for (int round = 0; round < 2 && rc == SPAL_OK; ++round) {      // round 0 also settles the clocks
        for (int cand = 0; cand < 4 && rc == SPAL_OK; ++cand) {
            if (walking_is_slide) { p.slide_on = cand & 1; p.slide_fill_ok = 1; p.persistent = 0; }
            else p.persistent = cand & 1;
            p.nt_store = (cand >> 1) & 1;
            float ms = 0.f;
            timed(iters, &ms);
            if (rc == SPAL_OK && round == 1) {
                a->tuned_us[cand] = ms * 1e3f;
                if (ms < best_ms) { best_ms = ms; best = cand; }
                if (cand == planned) planned_ms = ms;
            }
        }
    }
    // (a form has to beat the planned one by 1 %: at config 3 the two forms measure within 0.1 us of each other on some boxes,
    //  and the one-super-tile form picked on such a margin then ran 4 % slower over the timed launches than the sliding form does)
    if (planned_ms <= 1.01f * best_ms) best = planned;
    if (walking_is_slide) { p.slide_on = best & 1; p.slide_fill_ok = 1; p.persistent = 0; }
    else p.persistent = best & 1;
    p.user_persistent = true;   // measured: a later re-plan keeps it
    p.nt_store = (best >> 1) & 1;
    // ---- 1b. row records (csr_rowrec.hpp) against col16 on the kept form: 5 % fewer bytes per f64 row of 14 entries for a
    // decode per lane; kept where that wins by 1 % (the results are bit-identical)
    a->rowrec_us[0] = a->rowrec_us[1] = 0.f;
    const bool packed = p.valpack && a->d_valpack;
    if (rc == SPAL_OK && walking_is_slide && p.slide_on && p.rowrec && a->d_rowrec) {
        float ms[2] = {0.f, 0.f};
        const int vp = p.valpack_on;
        p.valpack_on = 0;   // (the records on their own: the packed values are stage 1c's)
        for (int round = 0; round < 2 && rc == SPAL_OK; ++round)
            for (int on = 0; on < 2 && rc == SPAL_OK; ++on) { p.rowrec_on = on; timed(iters, &ms[on]); }
        p.valpack_on = vp;
        if (rc == SPAL_OK) {
            a->rowrec_us[0] = ms[0] * 1e3f; a->rowrec_us[1] = ms[1] * 1e3f;
            p.rowrec_on = ms[1] <= 0.99f * ms[0] ? 1 : 0;
        }
    }
    // ---- 1c. packed values (csr_valpack.hpp) against the values on the record form: 96 instead of 112 B per f64 row of 14
    // entries for a fixed-point decode per lane; kept where that wins by 1 % (the results are bit-identical)
    a->valpack_us[0] = a->valpack_us[1] = 0.f;
    // (the packed form rides on the records: it is timed with them against whatever stage 1b kept, and brings them along)
    if (rc == SPAL_OK && walking_is_slide && p.slide_on && p.rowrec && a->d_rowrec && packed) {
        float ms[2] = {0.f, 0.f};
        const int rr = p.rowrec_on;
        for (int round = 0; round < 2 && rc == SPAL_OK; ++round)
            for (int on = 0; on < 2 && rc == SPAL_OK; ++on) {
                p.valpack_on = on;
                p.rowrec_on = on ? 1 : rr;
                timed(iters, &ms[on]);
            }
        p.valpack_on = 0;
        p.rowrec_on = rr;
        if (rc == SPAL_OK) {
            a->valpack_us[0] = ms[0] * 1e3f; a->valpack_us[1] = ms[1] * 1e3f;
            if (ms[1] <= 0.99f * ms[0]) p.valpack_on = p.rowrec_on = 1;
        }
    }
    // ---- 2. where the 16-bit columns lie relative to the values (two streams out of one class of region
    // disturb each other, +12 us at config 3; out of two classes they do not): the columns are copied into blocks of
    // 1 GiB taken one after the other from the device's memory, the kernel is timed on each, the fastest place is kept
    // (round 2 re-allocated the 1.1 GB values array up to 12 times and, the candidates lying side by side in one
    // region, often found nothing).  `place_tries` blocks (default 8: ~25 ms), up to three times as many while nothing better turns up.
    // Round 4: the candidates are the process's placement blocks (spal_csr_alloc_vectors' walk found and kept them: at most
    // two, no hipMalloc here), the columns become a PIECE of the one that wins by 1 % and more.
    int tries = p.place_tries;
    if (const char *e = getenv("SPAL_PLACE_TRIES")) tries = atoi(e);
    // (the column array the kept form streams: the row records, or col16)
    const bool recs = rowrec_runs(a) && walking_is_slide && p.slide_on;
    void **const slot = recs ? (void **)&a->d_rowrec : (void **)&a->d_col16;
    int *const placed = recs ? &a->rowrec_placed : &a->col16_placed;
    const size_t cbytes = recs ? a->rowrec_bytes : a->d_col16 ? (size_t)a->cap_entries * sizeof(uint16_t) : 0;
    if (rc == SPAL_OK && tries > 0 && cbytes >= ((size_t)64 << 20) && !*placed) {
        const int n = std::max(4, iters / 4);
        float cur_ms = 0.f;
        timed(n, &cur_ms);
        a->place_us[0] = cur_ms * 1e3f;
        void *const original = *slot;
        std::vector<void *> cand;
        std::vector<float> ms_of;
        const int kept = place_block_count(a->device);
        for (int k = 0; k < kept && k < tries && rc == SPAL_OK; ++k) {
            void *b = place_alloc(a->device, k, cbytes);
            if (!b) continue;
            hipError_t e = hipMemcpyAsync(b, original, cbytes, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) { place_free(a->device, b); rc = fail(SPAL_ERR_HIP, "spal_csr_autotune: %s", hipGetErrorString(e)); break; }
            *slot = b;
            float ms = 0.f;
            timed(n, &ms);
            cand.push_back(b); ms_of.push_back(ms);
            ++a->place_tried;
        }
        int best = -1;
        for (size_t k = 0; k < ms_of.size(); ++k)
            if (ms_of[k] < 0.99f * cur_ms && (best < 0 || ms_of[k] < ms_of[(size_t)best])) best = (int)k;
        (void)hipStreamSynchronize(st);
        *slot = best >= 0 ? cand[(size_t)best] : original;
        for (size_t k = 0; k < cand.size(); ++k)
            if ((int)k != best) place_free(a->device, cand[k]);
        if (best >= 0) { (void)dev_free(original); *placed = 1; }
        a->place_us[1] = (best >= 0 ? ms_of[(size_t)best] : cur_ms) * 1e3f;
    }
    return rc;
}

}  // namespace spal

using namespace spal;

extern "C" {

int spal_csr_alloc_vectors(spal_csr_t a, void **x_dev, void **y_dev, void *stream) {
    if (!a || !x_dev || !y_dev) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_alloc_vectors: null argument");
    DeviceGuard guard(a->device);
    if (guard.status != SPAL_OK) return guard.status;
    SPAL_TRY(csr_ensure_plan(a, nullptr, false));
    std::lock_guard<std::mutex> lock(a->mu);
    const size_t es = (size_t)a->elem_size;
    auto up = [](size_t v) { return (v + 4095) & ~(size_t)4095; };
    const size_t xb = up(std::max<uint64_t>(a->ncols, 1) * es), yb = up(std::max<uint64_t>(a->nrows, 1) * es);
    if (a->d_vec_block) {
        *x_dev = (char *)a->d_vec_block + a->vec_x_off;
        *y_dev = (char *)a->d_vec_block + a->vec_y_off;
        return SPAL_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    // small products, empty matrices, row-block handles: nothing to place -- a block of their own, exactly as large as needed
    size_t walk_min = (size_t)256 << 20;    // matrices the caches do not hold
    if (const char *e = getenv("SPAL_WALK_MIN_BYTES")) walk_min = (size_t)strtoull(e, nullptr, 10);
    const bool walk = a->parts.empty() && a->nnz != 0 && (size_t)a->nnz * (es + 2) >= walk_min && a->walk_max > 1 &&
                      xb + yb <= ((size_t)1 << 30);
    if (!walk) {
        void *b = nullptr;
        hipError_t e = hipMalloc(&b, up(xb + yb));
        if (e == hipSuccess) e = hipMemsetAsync(b, 0, xb + yb, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            if (b) (void)hipFree(b);
            return fail(e == hipErrorOutOfMemory ? SPAL_ERR_OUT_OF_MEMORY : SPAL_ERR_HIP, "spal_csr_alloc_vectors: %s", hipGetErrorString(e));
        }
        a->d_vec_block = b; a->vec_block_owned = 1; a->vec_x_off = 0; a->vec_y_off = xb;
        a->walk_blocks = 1; a->walk_probes = 0;
        *x_dev = (char *)b; *y_dev = (char *)b + xb;
        return SPAL_OK;
    }
    // Where x and y lie relative to the matrix stream decides +-5 - 12 % of a product.  The process keeps a few
    // PLACEMENT BLOCKS of 1 GiB per device (place_*): the FIRST handle that asks walks the device's memory -- blocks taken
    // one after the other, its kernel timed into a candidate y in each, at most `walk_blocks` (8 GiB) held at once -- and
    // keeps the block where it ran fastest and, when a second class of region showed (3 % apart), the one where it ran
    // slowest; the others go back.  Every LATER handle times itself in the kept blocks only (no hipMalloc, two probes) and
    // takes its vectors -- and, in the autotune, its 16-bit columns -- as PIECES of them: no handle keeps a GiB for 160 MB.
    SetupTimer timer;
    int rc = SPAL_OK;
    auto hip_failed = [&](hipError_t e) { return fail(SPAL_ERR_HIP, "spal_csr_alloc_vectors: %s", hipGetErrorString(e)); };
    auto probe = [&](void *xc, float *us_out) {           // the handle's kernel, x and y at xc: 3 launches untimed, 8 timed
        void *yc = (char *)xc + xb;
        float ms = 0.f;
        const hipError_t e = hipMemsetAsync(xc, 0, xb + yb, st);   // x = 0: the time of a product does not depend on the values
        rc = e != hipSuccess ? hip_failed(e)
                             : timer.run(st, 3, 8, [&] { return csr_launch(a, xc, yc, st); }, &ms, "spal_csr_alloc_vectors");
        *us_out = ms * 1e3f / 8.f;
    };
    std::vector<float> us;          // per candidate
    std::vector<void *> piece;      // its x (a piece of a placement block)
    a->walk_blocks = 0;
    a->walk_probes = 0;
    // (i) the process's blocks
    const int kept = place_block_count(a->device);
    for (int k = 0; k < kept && rc == SPAL_OK; ++k) {
        void *pc = place_alloc(a->device, k, xb + yb);
        if (!pc) continue;
        float t = 0.f;
        probe(pc, &t);
        piece.push_back(pc); us.push_back(t);
        ++a->walk_probes;
    }
    // (ii) the walk, once per process and device (or when the kept blocks are full)
    if ((!place_walked(a->device) || piece.empty()) && rc == SPAL_OK) {
        const size_t block = (size_t)1 << 30;
        std::vector<void *> fresh;
        std::vector<float> fresh_us;
        for (int k = 0; k < a->walk_max && rc == SPAL_OK; ++k) {
            void *b = nullptr;
            if (hipMalloc(&b, block) != hipSuccess) { (void)hipGetLastError(); break; }   // the device is full: what we have
            float t = 0.f;
            probe(b, &t);
            fresh.push_back(b); fresh_us.push_back(t);
            ++a->walk_blocks; ++a->walk_probes;
        }
        if (rc == SPAL_OK && !fresh.empty()) {
            size_t lo = 0, hi = 0;
            for (size_t k = 1; k < fresh.size(); ++k) {
                if (fresh_us[k] < fresh_us[lo]) lo = k;
                if (fresh_us[k] > fresh_us[hi]) hi = k;
            }
            const bool two = fresh_us[hi] > 1.03f * fresh_us[lo];
            for (size_t k = 0; k < fresh.size(); ++k) {
                if (k == lo || (two && k == hi)) {
                    place_adopt(a->device, fresh[k], block);
                    void *pc = place_alloc(a->device, place_block_count(a->device) - 1, xb + yb);   // (its start: where it was timed)
                    piece.push_back(pc); us.push_back(fresh_us[k]);
                } else {
                    (void)hipFree(fresh[k]);
                }
            }
            place_set_walked(a->device);
            if (getenv("SPAL_WALK_DEBUG")) {
                fprintf(stderr, "[spal walk] us per product by new block:");
                for (float t : fresh_us) fprintf(stderr, " %.1f", t);
                fprintf(stderr, "  -> kept %zu%s\n", lo, two ? " and the slowest" : "");
            }
        } else {
            for (void *b : fresh) (void)hipFree(b);
        }
    }
    if (rc == SPAL_OK) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = hip_failed(e);
    }
    size_t best = 0;
    for (size_t k = 1; k < us.size(); ++k) if (us[k] < us[best]) best = k;
    const bool ok = rc == SPAL_OK && !piece.empty() && piece[best] != nullptr;
    for (size_t k = 0; k < piece.size(); ++k)
        if (!ok || k != best) place_free(a->device, piece[k]);
    if (rc != SPAL_OK) return rc;
    if (!ok) return fail(SPAL_ERR_OUT_OF_MEMORY, "spal_csr_alloc_vectors: %s", "no device memory for the vectors");
    a->d_vec_block = piece[best];
    a->vec_block_owned = 0;
    a->vec_x_off = 0;
    a->vec_y_off = xb;
    a->walk_us[0] = us[best];
    a->walk_us[1] = *std::max_element(us.begin(), us.end());
    if (getenv("SPAL_WALK_DEBUG")) {
        fprintf(stderr, "[spal walk] us per product by candidate:");
        for (float t : us) fprintf(stderr, " %.1f", t);
        fprintf(stderr, "  -> %zu (%d new blocks, %d probes)\n", best, a->walk_blocks, a->walk_probes);
    }
    *x_dev = (char *)a->d_vec_block + a->vec_x_off;
    *y_dev = (char *)a->d_vec_block + a->vec_y_off;
    return SPAL_OK;
}

int spal_csr_autotune_f64(spal_csr_t a, const double *x_dev, double *y_dev, void *stream, int iters) {
    return csr_autotune<double>(a, x_dev, y_dev, stream, iters);
}
int spal_csr_autotune_f32(spal_csr_t a, const float *x_dev, float *y_dev, void *stream, int iters) {
    return csr_autotune<float>(a, x_dev, y_dev, stream, iters);
}

}  // extern "C"
