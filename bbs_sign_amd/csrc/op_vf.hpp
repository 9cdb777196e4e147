// Host orchestration of one batched operation (template over the curve); instantiated by the
// per-curve translation units tu_*.hip so the library builds in parallel.
#pragma once
#include "ops_decl.hpp"

// ---- verify ------------------------------------------------------------------------------------
template <class C>
struct VfJob : JobBase<C> {
    using JobBase<C>::JobBase;
    VfArgs<C> a{};
    PairArgs<C> pa{};
    VfIngestArgs<C> ingest{};
    VfOctArgs<C> oct{};               // wire form only
    MsgHashArgs mh{};                 // raw-message form only
    BvState<C> bv{};                  // batch verification only
    PairedJobForm<C> jf{};            // the job's form (job_form.hpp)
};
constexpr const char* VF_SCALARS[4] = {"vf_scalars", "vf_scalars_mixed", "vf_scalars_keyed", "vf_scalars_keyed_mixed"};

// KEYED (bbs_*_keyed_*, instantiated in tu_vfk_*.hip): item i is verified under key key_index[i] of the context's key set
// (keyed.hpp); the fused pairing kernel in both job forms; bbs_ctx_set_batch_verification does not apply,
// bbs_ctx_set_keyed_batch_verification puts the combination per key in front of it
template <class C, bool KEYED>
int vf_upload(Ctx<C>* ctx, size_t n, const VfIn& in, bbs_job** out) {
    constexpr int N = C::FpP::N;
    constexpr int NC = C::FpP::NC;
    constexpr int FPB = 4 * NC;
    Form form;
    if (const int rcf = decide_form<KEYED>(ctx, FormOp::Verify, n, in.key_index, form, KEYED && in.job_keys)) return rcf;
    if (!out || (n && ((!in.signatures && !in.signature_octets) || !in.msg_off))) return BBS_E_ARG;
    if (ctx->use()) return BBS_E_HIP;
    const int L = ctx->L;
    const bool wire = in.signature_octets != nullptr;
    const size_t rec = wire ? (size_t)FPB + 32 : (size_t)2 * FPB + 32;
    const uint8_t* sigs = wire ? in.signature_octets : in.signatures;
    auto job = std::unique_ptr<VfJob<C>>(new VfJob<C>(ctx));
    job->n = n;
    job->jf.form = form;
    std::vector<uint32_t> kwords;     // keyed: key indexes and pairing order, in the staging image
    size_t kwords_at = 0;
    if constexpr (KEYED) {
        if (const int rck = job_keys_begin<C>(job.get(), ctx, in.job_keys, in.n_keys, in.pk_octets, job->jf)) return rck;
        keyed_order<C>(job.get(), ctx, n, in.key_index, job->jf, kwords);
    }
    // the batch as one staging image, one asynchronous copy; checks, range checks and the SoA transposition on the
    // device (stage VfIngest), as for proof_verify
    const bool raw = in.msg_byte_off != nullptr;
    RaggedIn ms{in.msg_off, in.messages, 32}, hb{in.hdr_off, in.headers, 1};
    ms.offsets_only = raw;
    if (!ms.measure(n) || !hb.measure(n) || hb.total > 0xF0000000ull) return BBS_E_ARG;
    RaggedIn mb{};
    size_t nm;
    if (!raw_message_section(ms, in.msg_byte_off, in.msg_bytes, mb, nm)) return BBS_E_ARG;
    if (int rc0 = stage_image(job.get(), n, sigs, rec, {&ms, &hb}, raw ? &mb : nullptr, nm, KEYED ? &kwords : nullptr, &kwords_at)) return rc0;
    const uint8_t* dimg = job->d_raw.template as<uint8_t>();
    if constexpr (KEYED) keyed_bind<C>(job->jf, n, reinterpret_cast<const uint32_t*>(dimg + kwords_at));
    int rc = BBS_OK;
    const size_t Lw = (size_t)std::max(L, 1), nn = std::max<size_t>(n, 1);
    VfArgs<C>& a = job->a;
    a.n = n; a.L = L; a.cc = ctx->d_consts.template as<CtxConsts<C>>();
    a.glv = glv_flag<C>(ctx, wire);
    uint32_t* sig_a = job->template scratch<uint32_t>((size_t)2 * NC * nn, rc);
    uint32_t* sig_e = job->template scratch<uint32_t>((size_t)8 * nn, rc);
    uint32_t* smsgs = job->template scratch<uint32_t>(Lw * 8 * nn, rc);
    uint32_t* offs = job->template scratch<uint32_t>(2 * nn, rc);
    if (rc) return rc;
    a.sig_a = sig_a; a.sig_e = sig_e; a.msgs = smsgs;
    a.hdr_off = offs; a.hdr_len = offs + nn; a.hdr_bytes = dimg + hb.at_data;
    a.fscal = job->template scratch<uint32_t>((size_t)(L + 2) * 8 * n, rc);
    a.partials = job->template scratch<uint32_t>((size_t)VF_NPARTS * 3 * N * n, rc);
    a.aff = job->template scratch<uint32_t>((size_t)2 * 2 * N * n, rc);
    a.fmiller = job->template scratch<uint32_t>((size_t)2 * 12 * N * n, rc);
    a.vtab = job->template scratch<uint32_t>((size_t)G1_TAB * 2 * N * nn, rc);
    if (rc) return rc;
    if ((rc = job->finish_setup_device())) return rc;
    a.status = job->d_status.template as<int8_t>();
    VfIngestArgs<C>& ia = job->ingest;
    ia.n = n; ia.L = L; ia.dst_too_long = ctx->dst_too_long ? 1 : 0; ia.has_sig = 1;
    ia.rec = wire ? nullptr : reinterpret_cast<const uint32_t*>(dimg);
    ia.oct = nullptr; ia.pcode = nullptr; ia.msg_dst_too_long = 0;
    if (wire) {
        int8_t* pcode = job->template scratch<int8_t>(nn, rc);
        if (rc) return rc;
        VfOctArgs<C>& oa = job->oct;
        oa.n = n; oa.oct = dimg; oa.sig_a = sig_a; oa.pcode = pcode;
        if (rt::launch<VfOctDecode<C>>(job->stream(), oa, n)) return BBS_E_HIP;
        ia.oct = dimg; ia.pcode = pcode;
    }
    ia.m_off = reinterpret_cast<const uint64_t*>(dimg + ms.at_off); ia.hdr_off64 = reinterpret_cast<const uint64_t*>(dimg + hb.at_off);
    ia.m = reinterpret_cast<const uint32_t*>(dimg + ms.at_data);
    if (raw) {
        ia.m = hash_raw_messages<C>(job.get(), ctx, mb, nm, job->mh, ia.msg_dst_too_long, rc);
        if (rc) return rc;
    }
    ia.sig_a = sig_a; ia.sig_e = sig_e; ia.msgs = smsgs; ia.hdr_off = offs; ia.hdr_len = offs + nn;
    ia.status0 = job->d_status0.template as<int8_t>();
    if ((rc = form_bind<C>(job.get(), ctx, nn, job->jf))) return rc;
    if constexpr (KEYED) {
        if ((rc = job_keys_launch<C>(job.get(), ctx, job->jf, job->jf.unit))) return rc;
    }
    if ((rc = launch_ingest<VfIngest<C>, VfIngestMixed<C>>(job.get(), job->jf, ia, n))) return rc;
    if constexpr (KEYED) {
        if ((rc = paired_keyed_gate<C>(job.get(), n, job->jf, ia.status0))) return rc;
    }
    PairArgs<C>& pa = job->pa;
    pa.n = n; pa.cc = a.cc; pa.pa = a.aff; pa.pb = a.aff + (size_t)2 * N * n; pa.negate_b = 0;
    pa.canonical = 0; pa.gate_arr = a.status; pa.gate = ST_PAIRING; pa.out = a.status; pa.fmiller = a.fmiller;
    VfJob<C>* j = job.get();
    // e * A needs only what the ingest stage left: it runs on the job's side stream beside the scalars and the fixed-base
    // chunks (critical path 3.0 instead of 0.13 + 0.9 + 3.0 ms).  In both forms: with 6 / 8 / 12 resident jobs in flight
    // 1.75 / 1.79 / 1.81 M verify/s against 1.64 / 1.71 / 1.81 with the job kept to one stream
    // (profiles/r05_e_verify_var_mul_side_stream.log).  Except batch verification's throughput form, whose jobs are kept alive
    // by the dozen and must own ONE hardware queue each (32 in flight: 4.2 M/s on one stream, 3.1 M/s on two).
    const int side = (!KEYED && ctx->batch_verify && !job->latency_form) ? 0 : 1;
    j->stages.push_back({"vf_var_mul", [j, side]() { return rt::launch<VfVarMul<C>>(side ? j->stream_aux(1) : j->stream(), j->a, j->n); }, side, 0});
    add_scalar_stage<C, KEYED, VfScalars<C>, VfScalarsIn>(j, VF_SCALARS);
    j->stages.push_back({"vf_fixed_chunks", [j]() { return rt::launch<VfFixedChunk<C>>(j->stream(), j->a, j->n * (size_t)NFIX); }});
    j->stages.push_back({"vf_combine", [j]() { return rt::launch<VfCombine<C>>(j->stream(), j->a, j->n); }, 0, 1});
    if constexpr (KEYED) {
        // keyed batch verification (bbs_ctx_set_keyed_batch_verification): the combination per key and its decision go in front of
        // the per-item kernel, which then computes only the items still pending (nothing is added where no group formed)
        if ((rc = add_keyed_bv_stages<C>(j, ctx, &j->jf, n, a.cc, pa.pa, pa.pb, 0, a.status))) return rc;
        add_keyed_pairing_stages<C>(j, &j->jf, &j->pa, 0);
    } else if (!ctx->batch_verify) {
        add_pairing_stages<C>(j, &j->pa, 0, "pair_miller", "pair_final_exp", "pairing_6lane");
    } else {
        // e(A, W) e(e A - B, BP2) == 1 for all pending items at once: A and e A - B are in a.aff (Montgomery)
        // (the second point is computed by vf_combine, so here the combination follows the MSM chain on the main stream)
        if ((rc = add_batch_combination<C>(j, &j->bv, ctx, n, a.cc, a.aff, a.aff + (size_t)2 * N * n, 0, a.status, ST_PAIRING, 0, 0))) return rc;
        add_batch_decision<C>(j, &j->bv, &j->pa, 0);
    }
    *out = job.release();
    return BBS_OK;
}

// ---- bbs_selftest_segmented_sums -------------------------------------------------------------------------------------------
// Stages 2 - 3 of keyed batch verification alone (pippenger.hpp): n points in group order, 16 digit rows, G groups given as
// runs of the input -> the 16 window sums of every group.  The bv order (runs at multiples of 4, segments of at most PIP_TILE
// items) is built here as keyed_bv_plan builds it.  Product library: k_pip_window_seg; host twin: PipGroupSumsHost.
// Instantiated in the keyed verify units, where the kernel lives.
template <class C>
int selftest_segmented_sums(Ctx<C>* ctx, size_t n, const uint8_t* points_affine, const uint8_t* digits, size_t n_groups,
                            const uint64_t* group_first, const uint64_t* group_count, uint8_t* out_affine) {
    constexpr int N = C::FpP::N;
    constexpr int FPB = 4 * C::FpP::NC;
    constexpr int NW = 16;
    using P = typename C::FpP;
    if (!n_groups) return BBS_OK;
    if (!group_first || !group_count || !out_affine || (n && (!points_affine || !digits))) return BBS_E_ARG;
    if (n > 0x7FFFFFFFull || n_groups > 0x00FFFFFFull) return BBS_E_ARG;
    std::vector<uint32_t> segs, gseg(2 * n_groups), grun(2 * n_groups);
    size_t n_pos = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (group_first[g] > n || group_count[g] > n - group_first[g]) return BBS_E_ARG;
        const uint32_t cnt = (uint32_t)group_count[g];
        gseg[2 * g] = (uint32_t)(segs.size() / 3);
        for (uint32_t off = 0; off < cnt; off += PIP_TILE) {
            segs.push_back((uint32_t)n_pos + off); segs.push_back(std::min<uint32_t>(PIP_TILE, cnt - off)); segs.push_back((uint32_t)g);
        }
        gseg[2 * g + 1] = (uint32_t)(segs.size() / 3) - gseg[2 * g];
        grun[2 * g] = (uint32_t)n_pos; grun[2 * g + 1] = cnt;
        n_pos += ((size_t)cnt + 3) & ~(size_t)3;
        if (n_pos > 0x7FFFFFF0ull) return BBS_E_ARG;
    }
    const size_t n_segs = segs.size() / 3, NV = (size_t)NW * n_groups;
    std::vector<uint32_t> hp(std::max<size_t>(n_pos, 1) * 2 * N, 0);
    std::vector<uint8_t> hd((size_t)NW * n_pos + 4, 0);
    for (size_t g = 0; g < n_groups; g++) {
        for (size_t k = 0; k < group_count[g]; k++) {
            const size_t i = group_first[g] + k, pos = grun[2 * g] + k;
            G1Aff<C> pt;
            if (!fe_from_le_bytes<P>(points_affine + i * 2 * FPB, pt.x) || !fe_from_le_bytes<P>(points_affine + i * 2 * FPB + FPB, pt.y)) return BBS_E_ARG;
            if (!g1a_on_curve<C>(pt)) return BBS_E_ARG;           // ((0, 0) is the identity)
            for (int j = 0; j < N; j++) { hp[pos * 2 * N + j] = pt.x.v[j]; hp[pos * 2 * N + N + j] = pt.y.v[j]; }
            for (int w = 0; w < NW; w++) hd[(size_t)w * n_pos + pos] = digits[(size_t)w * n + i];
        }
    }
    if (ctx->use()) return BBS_E_HIP;
    std::vector<uint32_t> tab(segs);
    if (tab.empty()) tab.push_back(0);
    const size_t o_gseg = tab.size(); tab.insert(tab.end(), gseg.begin(), gseg.end());
    const size_t o_grun = tab.size(); tab.insert(tab.end(), grun.begin(), grun.end());
    DevBuf dTab, dP, dD, dS, dOut;
    if (dTab.alloc(tab.size() * 4) || dP.alloc(hp.size() * 4) || dD.alloc(hd.size()) || dS.alloc(std::max<size_t>((size_t)3 * N * NW * n_segs, 1) * 4) ||
        dOut.alloc((size_t)2 * N * NV * 4)) return BBS_E_NOMEM;
    if (rt::h2d(dTab.p, tab.data(), tab.size() * 4, ctx->stream) || rt::h2d(dP.p, hp.data(), hp.size() * 4, ctx->stream) ||
        rt::h2d(dD.p, hd.data(), hd.size(), ctx->stream)) return BBS_E_HIP;
    PipSegArgs<C> a{};
    a.n_pos = n_pos; a.M = 1; a.NW = NW; a.n_segs = (uint32_t)n_segs; a.n_groups = (uint32_t)n_groups;
    a.segs = dTab.as<uint32_t>(); a.grp_seg = a.segs + o_gseg; a.grp_run = a.segs + o_grun;
    a.ppts = dP.as<uint32_t>(); a.dig = dD.as<uint8_t>(); a.seg_sums = dS.as<uint32_t>(); a.out = dOut.as<uint32_t>();
#ifdef BBS_HOST_TWIN
    if (rt::launch<PipGroupSumsHost<C>>(ctx->stream, a, NV)) return BBS_E_HIP;
#else
    if (rt::launch_pip_window_segs<C>(ctx->stream, a)) return BBS_E_HIP;
#endif
    if (rt::launch<PipGroupSums<C>>(ctx->stream, a, NV) || rt::sync(ctx->stream)) return BBS_E_HIP;
    std::vector<uint32_t> w((size_t)2 * N * NV);
    if (rt::d2h(w.data(), dOut.p, w.size() * 4, ctx->stream)) return BBS_E_HIP;
    for (size_t v = 0; v < NV; v++) {
        G1Aff<C> r;
        for (int j = 0; j < N; j++) { r.x.v[j] = w[(size_t)j * NV + v]; r.y.v[j] = w[(size_t)(N + j) * NV + v]; }
        uint8_t* o = out_affine + v * 2 * FPB;
        if (g1a_is_inf<C>(r)) std::memset(o, 0, 2 * FPB);
        else { fe_to_le_bytes<P>(r.x, o); fe_to_le_bytes<P>(r.y, o + FPB); }
    }
    return BBS_OK;
}

