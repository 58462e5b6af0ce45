// ivf_maint.h — host side of the resident re-partition (kernels_maint.h): fvdb_ivf_compact, fvdb_ivf_train_from,
// fvdb_ivf_assign_from, fvdb_ivf_refill_from, fvdb_ivf_maintenance_info.  Included at the end of fvdb_hip.cpp (same
// translation unit: it works on fvdb_ivf and reuses train_resident and assign_dev defined there).
//
// What crosses the host link is the list tables (8 bytes per 64-row block up, 4 bytes per list down and 8 up) and
// what the caller asks for: ids (8 bytes a row), clusters or positions (4 bytes a row).  Rows, norms and live bits
// stay in HBM.  The job holds the old pool and the new one until the move has finished; every allocation happens
// before anything of the destination index is touched, so FVDB_E_OOM leaves it as it was.
#pragma once

namespace {

struct DBufs {  // temporaries of one job, freed when it returns
  DBuf tab, hist, total, rank, inv, pos, ids, dx;
};

int maint_index_ok(fvdb_ivf* ivf) {
  if (!ivf) return FVDB_E_INVALID;
  if (ivf->glob_set) FAIL(ivf->ctx, FVDB_E_UNSUPPORTED, "a sharded index (global list sizes set) cannot be re-partitioned");
  if (ivf->total_rows >= (1ull << 31)) FAIL(ivf->ctx, FVDB_E_UNSUPPORTED, "too many rows");
  return FVDB_OK;
}

int maint_pair_ok(fvdb_ivf* dst, fvdb_ivf* src) {
  if (!dst || !src) return FVDB_E_INVALID;
  fvdb_ctx* ctx = dst->ctx;
  if (dst == src) FAIL(ctx, FVDB_E_INVALID, "dst and src must be different indexes");
  if (dst->d != src->d || dst->f16 != src->f16 || dst->pool.mirror != src->pool.mirror ||
      dst->ctx->device != src->ctx->device)
    FAIL(ctx, FVDB_E_INVALID, "dst and src must share d, row dtype and device");
  int rc = maint_index_ok(dst);
  return rc ? rc : maint_index_ok(src);
}

// Sequence map of `src` into holder->m_seq (and, for a compact, each row's destination into holder->m_dest).
int build_seq(fvdb_ivf* holder, fvdb_ivf* src, bool compact_dest, DBufs& T, uint64_t* host_bytes) {
  fvdb_ctx* ctx = holder->ctx;
  const uint64_t n = src->total_rows;
  std::vector<uint32_t> tab;  // [block nsb][seq0 nsb + 1][list nsb]
  uint32_t nsb = 0;
  for (uint32_t L = 0; L < src->nlist; ++L) nsb += cdiv(src->list_len[L], 64);
  tab.resize((size_t)nsb * 3 + 1);
  uint32_t *blk = tab.data(), *seq0 = blk + nsb, *lst = seq0 + nsb + 1;
  uint32_t s = 0, run = 0;
  for (uint32_t L = 0; L < src->nlist; ++L) {
    const uint32_t len = src->list_len[L];
    for (uint32_t b = 0; b * 64 < len; ++b, ++s) {
      blk[s] = src->list_blocks[L][b];
      seq0[s] = run;
      lst[s] = L;
      run += std::min<uint32_t>(64, len - b * 64);
    }
  }
  seq0[nsb] = run;
  if (run != n) FAIL(ctx, FVDB_E_INVALID, "list lengths and total_rows disagree");
  HIPCHK(ctx, T.tab.ensure(tab.size() * 4));
  HIPCHK(ctx, holder->m_seq.ensure(std::max<uint64_t>(n, 1) * 4));
  if (compact_dest) HIPCHK(ctx, holder->m_dest.ensure(std::max<uint64_t>(n, 1) * 4));
  if (nsb == 0) return FVDB_OK;
  HIPCHK(ctx, hipMemcpyAsync(T.tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  *host_bytes += tab.size() * 4;
  const uint32_t* d = T.tab.as<uint32_t>();
  hipLaunchKernelGGL(seq_map_kernel, dim3(cdiv((uint64_t)nsb * 64, 256)), dim3(256), 0, ctx->stream, d, d + nsb,
                     d + 2 * (size_t)nsb + 1, nsb, src->pool.valid(), holder->m_seq.as<uint32_t>(),
                     compact_dest ? holder->m_dest.as<uint32_t>() : (uint32_t*)nullptr);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // `tab` goes out of scope
  return FVDB_OK;
}

// rows [o, o + B) of the sequence in holder->m_seq -> out[B][d]
void launch_gather(fvdb_ivf* holder, fvdb_ivf* src, uint64_t o, uint32_t B, float* out) {
  const Pool& P = src->pool;
  const int mode = P.rm() ? GATHER_ROW_MAJOR : (P.esize == 4 ? GATHER_BLOCKED_F32 : GATHER_BLOCKED_F16);
  const uint32_t nch = (uint32_t)(P.block_bytes() / 1024);
  const void* rows = P.rm() ? (const void*)P.rm() : (const void*)P.data();
  hipLaunchKernelGGL(gather_seq_rows_kernel, dim3(cdiv((uint64_t)B * nch, 256)), dim3(256), 0, holder->ctx->stream, rows,
                     holder->m_seq.as<uint32_t>() + o, B, src->d, nch, mode, out);
}

// The job itself.  The first n rows of src's sequence (dst->m_seq) go to the lists named in dst->m_dest (kMaintNone
// = dropped); dst's lists become exactly those rows.  dst == src is the compact.  out_pos [n] and out_ids [rows kept]
// are optional host buffers.
int repartition(fvdb_ivf* dst, fvdb_ivf* src, uint64_t n, uint32_t* out_pos, uint64_t* out_ids, DBufs& T,
                fvdb_maintenance_info_t* info) {
  fvdb_ctx* ctx = dst->ctx;
  dst->mutations += 1;  // rows move: masks of dst are stale from here on
  const uint32_t nlist = dst->nlist;
  if (nlist > kRankMaxLists)
    FAIL(ctx, FVDB_E_UNSUPPORTED, "re-partition ranks destinations with one LDS counter per list: at most 16384 lists");
  StageTimer<2> clock;
  HIPCHK(ctx, clock.create());
  std::vector<uint32_t> total(nlist, 0);
  if (n > 0) {
    // tiles of the sequence; the per-tile counts take tiles * nlist * 4 bytes, kept under 256 MiB
    uint32_t tile = 4096;
    while ((uint64_t)cdiv(n, tile) * nlist * 4 > (256ull << 20)) tile *= 2;
    const uint32_t tiles = cdiv(n, tile);
    HIPCHK(ctx, T.hist.ensure((size_t)tiles * nlist * 4));
    HIPCHK(ctx, T.total.ensure((size_t)nlist * 4));
    HIPCHK(ctx, T.rank.ensure(n * 4));
    clock.begin(ctx->stream);
    const uint32_t* dest = dst->m_dest.as<uint32_t>();
    hipLaunchKernelGGL(rank_hist_kernel, dim3(tiles), dim3(256), (size_t)nlist * 4, ctx->stream, dest, (uint32_t)n, tile,
                       nlist, T.hist.as<uint32_t>());
    hipLaunchKernelGGL(rank_scan_kernel, dim3(cdiv(nlist, 256)), dim3(256), 0, ctx->stream, T.hist.as<uint32_t>(), tiles,
                       nlist, T.total.as<uint32_t>());
    hipLaunchKernelGGL(rank_assign_kernel, dim3(tiles), dim3(64), (size_t)nlist * 4, ctx->stream, dest, (uint32_t)n, tile,
                       nlist, T.hist.as<uint32_t>(), T.rank.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(total.data(), T.total.p, (size_t)nlist * 4, hipMemcpyDeviceToHost, ctx->stream));
    info->ms_ranks += clock.end(ctx->stream);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    info->host_bytes += (uint64_t)nlist * 4;
  }
  // the fresh pool: the blocks of a list are consecutive, lists in ascending order
  std::vector<uint32_t> tab((size_t)nlist * 2);  // [first block of the list][rows before the list]
  uint64_t blocks = 0, rows_out = 0;
  for (uint32_t L = 0; L < nlist; ++L) {
    tab[L] = (uint32_t)blocks;
    tab[nlist + L] = (uint32_t)rows_out;
    blocks += cdiv(total[L], 64);
    rows_out += total[L];
  }
  if (blocks >= (1ull << 26) || rows_out > n) FAIL(ctx, FVDB_E_UNSUPPORTED, "pool too large");
  Pool fresh;
  if (blocks > 0) {
    HIPCHK(ctx, T.tab.ensure(tab.size() * 4));
    HIPCHK(ctx, T.inv.ensure(blocks * 64 * 4));
    if (out_pos) HIPCHK(ctx, T.pos.ensure(n * 4));
    if (out_ids) HIPCHK(ctx, T.ids.ensure(rows_out * 8));
    if (dst != src && src->d_xmax.p && !dst->d_xmax.p) {
      HIPCHK(ctx, dst->d_xmax.ensure(4));
      HIPCHK(ctx, hipMemsetAsync(dst->d_xmax.p, 0, 4, ctx->stream));
    }
    // nothing is cleared: the move stage writes all 64 lanes of every block, tail lanes as zeros (pool_buffers says
    // why they must be finite)
    HIPCHK(ctx, pool_buffers(dst->pool, (uint32_t)blocks, /*carry=*/false, ctx->stream, &fresh));
    // from here on a failure is a HIP error, not a shortage
    HIPCHK(ctx, hipMemcpyAsync(T.tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    info->host_bytes += tab.size() * 4;
    clock.begin(ctx->stream);
    HIPCHK(ctx, hipMemsetAsync(T.inv.p, 0xFF, blocks * 64 * 4, ctx->stream));
    const Pool& S = src->pool;
    hipLaunchKernelGGL(place_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, dst->m_dest.as<uint32_t>(),
                       T.rank.as<uint32_t>(), dst->m_seq.as<uint32_t>(), (uint32_t)n, nlist, T.tab.as<uint32_t>(),
                       T.tab.as<uint32_t>() + nlist, S.ids(), (uint32_t)(blocks * 64), (uint32_t)rows_out,
                       T.inv.as<uint32_t>(), out_pos ? T.pos.as<uint32_t>() : (uint32_t*)nullptr,
                       out_ids ? T.ids.as<uint64_t>() : (uint64_t*)nullptr);
    const uint32_t nch = (uint32_t)(S.block_bytes() / 1024);
    if (S.rm() && fresh.rm())
      hipLaunchKernelGGL(move_rows_rm_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, T.inv.as<uint32_t>(),
                         (const float4*)S.rm(), S.ids(), S.norms(), S.valid(), S.d4, (float4*)fresh.data(), (float4*)fresh.rm(),
                         fresh.half(), fresh.ids(), fresh.norms(), fresh.valid());
    else
      hipLaunchKernelGGL(move_rows_blocked_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream,
                         T.inv.as<uint32_t>(), (const uint4*)S.data(), S.ids(), S.norms(), S.valid(), nch, (uint4*)fresh.data(),
                         fresh.ids(), fresh.norms(), fresh.valid());
    if (dst != src && src->d_xmax.p)
      hipLaunchKernelGGL(max_bits_kernel, dim3(1), dim3(64), 0, ctx->stream, src->d_xmax.as<uint32_t>(),
                         dst->d_xmax.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    info->ms_move += clock.end(ctx->stream);
    if (out_pos) HIPCHK(ctx, hipMemcpyAsync(out_pos, T.pos.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_ids) HIPCHK(ctx, hipMemcpyAsync(out_ids, T.ids.p, rows_out * 8, hipMemcpyDeviceToHost, ctx->stream));
    info->host_bytes += (out_pos ? n * 4 : 0) + (out_ids ? rows_out * 8 : 0);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // bytes of the move: the source rows once (through `rm` where the pool keeps it), every representation written
    const size_t bb = fresh.block_bytes();
    const uint64_t per_block_written = bb * (fresh.rm() ? 2 : 1) + (fresh.half() ? bb / 2 : 0) + 64 * 12 + 8;
    info->move_bytes += blocks * per_block_written + rows_out * ((uint64_t)bb / 64 + 12) + blocks * 64 * 4;
  } else if (out_pos && n) {
    std::fill(out_pos, out_pos + n, kMaintNone);
  }
  // swap
  if (blocks > 0) {
    dst->pool = std::move(fresh);
  } else {  // nothing survives: the lists are empty, the pool keeps its blocks for later appends
    dst->pool.used_blocks = 0;
    if (dst->pool.valid() && dst->pool.cap_blocks)
      HIPCHK(ctx, hipMemsetAsync(dst->pool.valid(), 0, (size_t)dst->pool.cap_blocks * 8, ctx->stream));
  }
  uint32_t b = 0;
  for (uint32_t L = 0; L < nlist; ++L) {
    const uint32_t nb = cdiv(total[L], 64);
    dst->list_blocks[L].resize(nb);
    for (uint32_t j = 0; j < nb; ++j) dst->list_blocks[L][j] = b++;
    dst->list_len[L] = total[L];
  }
  dst->total_rows = rows_out;
  dst->table_dirty = true;
  info->rows_in += n;
  info->rows_out += rows_out;
  return FVDB_OK;
}

void finish_info(fvdb_maintenance_info_t* m) {
  m->ms_total = m->ms_gather + m->ms_train + m->ms_assign + m->ms_ranks + m->ms_move;
}

}  // namespace

extern "C" {

int fvdb_ivf_compact(fvdb_ivf* ivf, uint64_t* removed, uint64_t* out_ids) {
  int rc = maint_index_ok(ivf);
  if (rc) return rc;
  fvdb_ctx* ctx = ivf->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t n = ivf->total_rows;
  ivf->m_info = fvdb_maintenance_info_t{};
  ivf->m_src = nullptr;
  ivf->m_assigned = false;
  if (removed) *removed = 0;
  if (n == 0) return FVDB_OK;
  DBufs T;
  rc = build_seq(ivf, ivf, true, T, &ivf->m_info.host_bytes);
  if (rc) return rc;
  rc = repartition(ivf, ivf, n, nullptr, out_ids, T, &ivf->m_info);
  ivf->m_seq.release();  // 8 bytes a row that nothing reads after the job
  ivf->m_dest.release();
  if (rc) return rc;
  finish_info(&ivf->m_info);
  if (removed) *removed = n - ivf->total_rows;
  return FVDB_OK;
}

int fvdb_ivf_train_from(fvdb_ivf* dst, fvdb_ivf* src, uint32_t max_iterations, uint64_t seed, fvdb_train_result* out) {
  int rc = maint_pair_ok(dst, src);
  if (rc) return rc;
  fvdb_ctx* ctx = dst->ctx;
  const uint64_t n = src->total_rows;
  rc = train_args_ok(dst, n, max_iterations);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(src->ctx->stream));
  dst->m_info = fvdb_maintenance_info_t{};
  dst->m_src = nullptr;
  dst->m_assigned = false;
  DBufs T;
  rc = build_seq(dst, src, false, T, &dst->m_info.host_bytes);
  if (rc) return rc;
  HIPCHK(ctx, T.dx.ensure(n * dst->d * 4));
  StageTimer<2> clock;
  HIPCHK(ctx, clock.create());
  clock.begin(ctx->stream);
  for (uint64_t o = 0; o < n; o += 1u << 20)  // a launch per 2^20 rows keeps the grid far below its limit
    launch_gather(dst, src, o, (uint32_t)std::min<uint64_t>(1u << 20, n - o), T.dx.as<float>() + o * dst->d);
  HIPCHK(ctx, hipGetLastError());
  dst->m_info.ms_gather += clock.end(ctx->stream);
  clock.begin(ctx->stream);
  rc = train_resident(dst, T.dx.as<float>(), n, max_iterations, seed, out);
  dst->m_info.ms_train += clock.end(ctx->stream);
  if (rc) return rc;
  dst->coarse_mode = src->coarse_mode;
  dst->scan_mode = src->scan_mode;
  dst->m_src = src;  // fvdb_ivf_assign_from of the same pair continues this job's figures
  finish_info(&dst->m_info);
  return FVDB_OK;
}

int fvdb_ivf_assign_from(fvdb_ivf* dst, fvdb_ivf* src, uint32_t* out_cluster, uint64_t* out_ids) {
  int rc = maint_pair_ok(dst, src);
  if (rc) return rc;
  fvdb_ctx* ctx = dst->ctx;
  if (!dst->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(src->ctx->stream));
  if (dst->m_src != src) dst->m_info = fvdb_maintenance_info_t{};
  dst->m_src = nullptr;
  dst->m_assigned = false;
  const uint64_t n = src->total_rows;
  DBufs T;
  rc = build_seq(dst, src, false, T, &dst->m_info.host_bytes);
  if (rc) return rc;
  HIPCHK(ctx, dst->m_dest.ensure(std::max<uint64_t>(n, 1) * 4));
  StageTimer<2> clock;
  HIPCHK(ctx, clock.create());
  const uint32_t step = 65536;  // assign_dev's own batch: the dense rows of one batch at a time, not the whole matrix
  for (uint64_t o = 0; o < n; o += step) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(step, n - o);
    HIPCHK(ctx, dst->s_in.ensure((size_t)B * dst->d * 4));
    clock.begin(ctx->stream);
    launch_gather(dst, src, o, B, dst->s_in.as<float>());
    dst->m_info.ms_gather += clock.end(ctx->stream);
    clock.begin(ctx->stream);
    rc = assign_dev(dst, dst->s_in.as<float>(), B, dst->m_dest.as<uint32_t>() + o);
    dst->m_info.ms_assign += clock.end(ctx->stream);
    if (rc) return rc;
  }
  if (n && out_cluster) {
    HIPCHK(ctx, hipMemcpyAsync(out_cluster, dst->m_dest.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    dst->m_info.host_bytes += n * 4;
  }
  if (n && out_ids) {
    HIPCHK(ctx, T.ids.ensure(n * 8));
    hipLaunchKernelGGL(gather_ids_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, dst->m_seq.as<uint32_t>(),
                       src->pool.ids(), (uint32_t)n, T.ids.as<uint64_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_ids, T.ids.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    dst->m_info.host_bytes += n * 8;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  dst->m_src = src;
  dst->m_rows = n;
  dst->m_assigned = true;
  finish_info(&dst->m_info);
  return FVDB_OK;
}

int fvdb_ivf_refill_from(fvdb_ivf* dst, fvdb_ivf* src, uint64_t n_rows, uint32_t* out_pos) {
  int rc = maint_pair_ok(dst, src);
  if (rc) return rc;
  fvdb_ctx* ctx = dst->ctx;
  if (!dst->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (!dst->m_assigned || dst->m_src != src || dst->m_rows != src->total_rows)
    FAIL(ctx, FVDB_E_INVALID, "fvdb_ivf_refill_from follows fvdb_ivf_assign_from of the same pair");
  if (dst->total_rows != 0) FAIL(ctx, FVDB_E_INVALID, "the destination lists must be empty");
  if (n_rows > dst->m_rows) FAIL(ctx, FVDB_E_INVALID, "n_rows exceeds the source's rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(src->ctx->stream));
  DBufs T;
  rc = repartition(dst, src, n_rows, out_pos, nullptr, T, &dst->m_info);
  dst->m_seq.release();  // as after a compact
  dst->m_dest.release();
  dst->m_src = nullptr;
  dst->m_rows = 0;
  dst->m_assigned = false;
  if (rc) return rc;
  finish_info(&dst->m_info);
  return FVDB_OK;
}

int fvdb_ivf_maintenance_info(fvdb_ivf* ivf, fvdb_maintenance_info_t* out) {
  if (!ivf || !out) return FVDB_E_INVALID;
  *out = ivf->m_info;
  return FVDB_OK;
}

}  // extern "C"
