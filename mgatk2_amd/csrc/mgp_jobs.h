// mgp_jobs.h — the one way from the row jobs (mgp_jobs.hip: the txt and HDF5 writers, the
// variant and coverage passes, everything that reads a finished run's rows) into the engine's
// context (internal). mgp_jobs.hip sees mgp_ctx as an incomplete type.
#pragma once
#include "../../include/mgpileup.h"
#include "mgp_qc.h"

struct RowJobs;  // the jobs' buffers, kept for the next call (mgp_jobs.hip); a context owns one
RowJobs* row_jobs_new();
void row_jobs_free(RowJobs* jobs);  // (on the device its buffers were allocated on)

// What a job gets of a context whose run has finished
struct RunRows {
    int device;
    hipStream_t stream;
    int32_t n_cells;
    mgp::txtgz::Rows rows;
    mgp::qc::Tn5 tn5;
    RowJobs* jobs;
};
// mgp_engine.hip. The view of `ctx`'s last run: null check, mgp_sync, hipSetDevice, then
// MGP_E_STATE with "`no_run` (mgp_run first)" when the context has no run. A table context
// (below) serves its loaded planes instead, once mgp_table_ready was called: no wide window,
// no u32 rows (null), one window over every position.
int run_rows(mgp_ctx* ctx, const char* no_run, RunRows* out);
// a context's device and jobs, no run needed (the *_fetch calls); ctx is not null
RowJobs* ctx_jobs(mgp_ctx* ctx, int* device);

// A table context (mgp_open_table) is the second producer of RunRows: its 16-bit planes are
// filled by the loader of mgp_table.hip, which a table context owns like its jobs.
struct TableLoad;
TableLoad* table_load_new();
void table_load_free(TableLoad* load);  // (on the device its buffers were allocated on)
struct TablePlanes {
    int device;
    hipStream_t stream;  // the table's own
    int32_t n_cells, mito_len;
    uint4* c16;     // [cells][mito_len]: 8 x u16 A_fwd, A_rev, ... T_rev
    uint32_t* t16;  // [cells][mito_len]: tn5 fwd | rev << 16
    uint16_t* d16;  // [cells][mito_len]
    TableLoad* load;
};
// mgp_engine.hip. The planes of the table `ctx`: null check, MGP_E_STATE when ctx is not a
// table or is ready already, hipSetDevice.
int table_planes(mgp_ctx* ctx, const char* who, TablePlanes* out);
