// ivf_rows.h — host side of the row gathers (kernels_rows.h): fvdb_ivf_get_rows, fvdb_ivf_get_rows_dev,
// fvdb_ivf_assign_from_store, fvdb_ivf_add_assigned_from_store.  Included at the end of fvdb_hip.cpp, after
// ivf_maint.h (same translation unit: it works on fvdb_ivf and fvdb_store, leases a scratch set like the blocking
// searches, and reuses assign_dev, append_staged and finish_info).
//
// A fetch only reads the index: it takes a leased scratch set (its own stream, s_fslots / s_frows), so any number of
// host threads may fetch beside searches in any slot.  The _from_store pair is a mutation like fvdb_ivf_add: it runs
// on the index's stream with the insert staging (s_slots for the row indices, s_in for the gathered rows), and after
// the gather it IS fvdb_ivf_assign / fvdb_ivf_add_assigned: the same assign_dev and append_staged read the same s_in.
#pragma once

namespace {

constexpr uint64_t kGatherStep = 1u << 20;  // rows per launch: the grid stays far below its limit

void launch_pool_gather(const fvdb_ivf* ivf, hipStream_t st, const uint32_t* slots_dev, uint64_t n, float* out, uint32_t ostride) {
  const Pool& P = ivf->pool;
  const uint32_t nch = (uint32_t)(P.block_bytes() / 1024);  // 16-byte chunks per row: d4 (f32), d8 (fp16)
  for (uint64_t o = 0; o < n; o += kGatherStep) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(kGatherStep, n - o);
    if (P.esize == 4)
      hipLaunchKernelGGL(pool_gather_rows_kernel<0>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, st, P.data(), P.rm(),
                         slots_dev + o, B, ivf->d, nch, out + o * ostride, ostride);
    else
      hipLaunchKernelGGL(pool_gather_rows_kernel<1>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, st, P.data(),
                         (const float*)nullptr, slots_dev + o, B, ivf->d, nch, out + o * ostride, ostride);
  }
}

// ostride: floats between output rows (d: tightly packed).  skips: a cluster of FVDB_NO_ROW leaves its output row alone.
int get_rows_common(fvdb_ivf* ivf, fvdb_ctx* on, const uint32_t* cluster, const uint32_t* pos, uint64_t n, float* out,
                    bool to_host, uint32_t ostride, bool skips) {
  if (!ivf) return FVDB_E_INVALID;
  if (ostride < ivf->d) FAIL(ivf->ctx, FVDB_E_INVALID, "output stride below the dimension");
  if (n == 0) return FVDB_OK;
  if (!cluster || !pos || !out) FAIL(ivf->ctx, FVDB_E_INVALID, "null argument");
  if (on && on->device != ivf->ctx->device) FAIL(ivf->ctx, FVDB_E_INVALID, "context of another device");
  std::vector<uint32_t> slots(n);
  for (uint64_t i = 0; i < n; ++i) {  // every location is checked before anything is enqueued
    if (skips && cluster[i] == FVDB_NO_ROW) {
      slots[i] = FVDB_NO_ROW;
      continue;
    }
    if (cluster[i] >= ivf->nlist || pos[i] >= ivf->list_len[cluster[i]]) FAIL(ivf->ctx, FVDB_E_NOT_FOUND, "no such row");
    slots[i] = ivf->list_blocks[cluster[i]][pos[i] >> 6] * 64 + (pos[i] & 63);
  }
  return on_lease(ivf, [&](const Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    IvfScratch& S = *E.S;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, S.s_fslots.ensure(n * 4));
    if (to_host) HIPCHK(ctx, S.s_frows.ensure(n * ivf->d * 4));
    HIPCHK(ctx, hipMemcpyAsync(S.s_fslots.p, slots.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (to_host) {
      launch_pool_gather(ivf, ctx->stream, S.s_fslots.as<uint32_t>(), n, S.s_frows.as<float>(), ostride);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(out, S.s_frows.p, n * ivf->d * 4, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      return FVDB_OK;
    }
    // Device form.  The slots go up on the set's own stream, which holds nothing else: waiting for it waits for that
    // copy alone (`slots` dies with this call).  The gather then runs on the caller's stream, and the set's stream
    // waits for it, so that the next holder of this set cannot overwrite s_fslots under the kernel.
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    hipStream_t st = on ? on->stream : ivf->ctx->stream;
    launch_pool_gather(ivf, st, S.s_fslots.as<uint32_t>(), n, out, ostride);
    HIPCHK(ctx, hipGetLastError());
    if (st != ctx->stream) {
      HIPCHK(ctx, S.fetch_done.create(hipEventDisableTiming));
      HIPCHK(ctx, hipEventRecord(S.fetch_done, st));
      HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, S.fetch_done, 0));
    }
    return FVDB_OK;
  });
}

int store_pair_ok(fvdb_ivf* ivf, fvdb_store* s, const uint32_t* rows, uint64_t n) {
  if (!ivf || !s) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ivf->ctx;
  if (s->d != ivf->d) FAIL(ctx, FVDB_E_DIM, "the store's rows have another dimension");
  if (s->ctx->device != ctx->device) FAIL(ctx, FVDB_E_INVALID, "the store lives on another device");
  if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (n && !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i)
    if (rows[i] >= s->rows) FAIL(ctx, FVDB_E_NOT_FOUND, "row out of range");
  return FVDB_OK;
}

// store rows `rows[n]` -> ivf->s_in ([n][d], what fvdb_ivf_assign / _add_assigned upload there); waits for the gather
int stage_from_store(fvdb_ivf* ivf, fvdb_store* s, const uint32_t* rows, uint64_t n, StageTimer<2>& clock) {
  fvdb_ctx* ctx = ivf->ctx;
  if (s->ctx != ctx) HIPCHK(ctx, hipStreamSynchronize(s->ctx->stream));  // rows written on the store's stream
  HIPCHK(ctx, ivf->s_in.ensure(n * ivf->d * 4));
  HIPCHK(ctx, ivf->s_slots.ensure(n * 4));
  clock.begin(ctx->stream);
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_slots.p, rows, n * 4, hipMemcpyHostToDevice, ctx->stream));
  for (uint64_t o = 0; o < n; o += kGatherStep) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(kGatherStep, n - o);
    if (s->f16())  // widened into the f32 staging: the lists round again, to the same values, if they are fp16 too
      hipLaunchKernelGGL(store_gather_rows_kernel<half_t>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, ctx->stream, (const half_t*)s->data, s->dpad,
                         ivf->s_slots.as<uint32_t>() + o, B, ivf->d, ivf->s_in.as<float>() + o * ivf->d, ivf->d, (uint32_t)s->rows);
    else
      hipLaunchKernelGGL(store_gather_rows_kernel<float>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, ctx->stream, (const float*)s->data, s->dpad,
                         ivf->s_slots.as<uint32_t>() + o, B, ivf->d, ivf->s_in.as<float>() + o * ivf->d, ivf->d, (uint32_t)s->rows);
  }
  HIPCHK(ctx, hipGetLastError());
  ivf->m_info.ms_gather += clock.end(ctx->stream);  // waits: `rows` is the caller's, and s_slots is written again by the append
  ivf->m_info.host_bytes += n * 4;
  return FVDB_OK;
}

}  // namespace

extern "C" {

int fvdb_ivf_get_rows(fvdb_ivf* ivf, const uint32_t* cluster, const uint32_t* pos, uint64_t n, float* out_rows) {
  return get_rows_common(ivf, nullptr, cluster, pos, n, out_rows, true, ivf ? ivf->d : 0, false);
}

int fvdb_ivf_get_rows_dev(fvdb_ivf* ivf, fvdb_ctx* on, const uint32_t* cluster, const uint32_t* pos, uint64_t n,
                          float* out_rows_dev) {
  return get_rows_common(ivf, on, cluster, pos, n, out_rows_dev, false, ivf ? ivf->d : 0, false);
}

int fvdb_ivf_get_rows_dev_strided(fvdb_ivf* ivf, fvdb_ctx* on, const uint32_t* cluster, const uint32_t* pos, uint64_t n,
                                  float* out_rows_dev, uint32_t out_stride) {
  return get_rows_common(ivf, on, cluster, pos, n, out_rows_dev, false, out_stride, true);
}

int fvdb_store_get_rows_dev(fvdb_store* s, fvdb_ctx* on, const uint32_t* rows_dev, uint64_t n, float* out_rows_dev, uint32_t out_stride) {
  if (!s) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : s->ctx;
  if (ctx->device != s->ctx->device) FAIL(s->ctx, FVDB_E_INVALID, "context of another device");
  if (out_stride < s->d) FAIL(s->ctx, FVDB_E_INVALID, "output stride below the dimension");
  if (n == 0) return FVDB_OK;
  if (!rows_dev || !out_rows_dev) FAIL(s->ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (uint64_t o = 0; o < n; o += kGatherStep) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(kGatherStep, n - o);
    if (s->f16())
      hipLaunchKernelGGL(store_gather_rows_kernel<half_t>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, ctx->stream, (const half_t*)s->data, s->dpad,
                         rows_dev + o, B, s->d, out_rows_dev + o * out_stride, out_stride, (uint32_t)s->rows);
    else
      hipLaunchKernelGGL(store_gather_rows_kernel<float>, dim3(cdiv(B, kRowsPerGroup)), dim3(256), 0, ctx->stream, (const float*)s->data, s->dpad,
                         rows_dev + o, B, s->d, out_rows_dev + o * out_stride, out_stride, (uint32_t)s->rows);
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_ivf_assign_from_store(fvdb_ivf* ivf, fvdb_store* store, const uint32_t* rows, uint64_t n, uint32_t* out_cluster) {
  int rc = store_pair_ok(ivf, store, rows, n);
  if (rc) return rc;
  fvdb_ctx* ctx = ivf->ctx;
  ivf->m_info = fvdb_maintenance_info_t{};
  ivf->m_store_job = false;
  if (n == 0) return FVDB_OK;
  if (!out_cluster) FAIL(ctx, FVDB_E_INVALID, "null output");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, ivf->s_clusters.ensure(n * 4));
  StageTimer<2> clock;
  HIPCHK(ctx, clock.create());
  rc = stage_from_store(ivf, store, rows, n, clock);
  if (rc) return rc;
  clock.begin(ctx->stream);
  rc = assign_dev(ivf, ivf->s_in.as<float>(), n, ivf->s_clusters.as<uint32_t>());
  ivf->m_info.ms_assign += clock.end(ctx->stream);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out_cluster, ivf->s_clusters.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ivf->m_info.host_bytes += n * 4;
  ivf->m_info.rows_in = n;
  ivf->m_store_job = true;  // fvdb_ivf_add_assigned_from_store continues these figures
  finish_info(&ivf->m_info);
  return FVDB_OK;
}

int fvdb_ivf_add_assigned_from_store(fvdb_ivf* ivf, fvdb_store* store, const uint32_t* rows, const uint64_t* ids, uint64_t n,
                                     const uint32_t* cluster, uint32_t* out_pos) {
  int rc = store_pair_ok(ivf, store, rows, n);
  if (rc) return rc;
  fvdb_ctx* ctx = ivf->ctx;
  if (!ivf->m_store_job) ivf->m_info = fvdb_maintenance_info_t{};
  ivf->m_store_job = false;
  if (n == 0) return FVDB_OK;
  if (!cluster) FAIL(ctx, FVDB_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i)
    if (cluster[i] >= ivf->nlist) FAIL(ctx, FVDB_E_INVALID, "cluster id out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  StageTimer<2> clock;
  HIPCHK(ctx, clock.create());
  rc = stage_from_store(ivf, store, rows, n, clock);
  if (rc) return rc;
  clock.begin(ctx->stream);
  rc = append_staged(ivf, ids, n, cluster, out_pos);
  ivf->m_info.ms_move += clock.end(ctx->stream);
  if (rc) return rc;
  ivf->m_info.host_bytes += n * 4 + (ids ? n * 8 : 0);  // slots up, ids up; positions come from host bookkeeping
  ivf->m_info.rows_in = ivf->m_info.rows_out = n;
  finish_info(&ivf->m_info);
  return FVDB_OK;
}

}  // extern "C"
