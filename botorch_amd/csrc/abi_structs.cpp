// Parameter-struct entry points of the C ABI (include/botorch_amd.h): each
// bo_<entry>_v validates the record's header and hands the record to
// bo_<entry>_impl in the kernel's own source file.  Host code only (g++): no
// device work of its own.
#include <cstdio>
#include <string>

#include "../../include/botorch_amd.h"

void bo_set_error(const char* fmt, ...);

namespace {

template <class T>
bool header_ok(const T* a, const char* name) {
  if (!a) {
    bo_set_error("%s: null argument struct", name);
    return false;
  }
  if (a->struct_size != sizeof(T) || a->abi_version != BO_ABI_VERSION) {
    bo_set_error("%s: struct size %u / ABI %u, library expects %zu / %d", name, a->struct_size,
                 a->abi_version, sizeof(T), BO_ABI_VERSION);
    return false;
  }
  return true;
}

}  // namespace

// Every record entry point: X(entry, record) stands for
// int bo_<entry>_v(const Bo<record>Args*, void* stream).
#define BO_RECORD_ENTRIES(X)                             \
  X(post_partials, PostPartials)     /* post.hip */      \
  X(qmc_finalize, QmcFinalize)       /* qmc.hip */       \
  X(qmc_backward, QmcBackward)       /* grad.hip */      \
  X(post_backward, PostBackward)                         \
  X(qehvi, Qehvi)                    /* qehvi.hip */     \
  X(qehvi_backward, Qehvi)                               \
  X(qehvi_feas, QehviFeas)                               \
  X(qehvi_feas_backward, QehviFeas)                      \
  X(qlogehvi, Qlogehvi)              /* qlogehvi.hip */  \
  X(qlogehvi_backward, Qlogehvi)                         \
  X(qmc_feas, QmcFeas)               /* qmc_feas.hip */  \
  X(qmc_feas_backward, QmcFeas)                          \
  X(kg, Kg)                          /* kg.hip */        \
  X(kg_backward, Kg)                                     \
  X(paths_eval, Paths)               /* paths.hip */     \
  X(paths_eval_backward, Paths)                          \
  X(jes, Jes)                        /* jes.hip */       \
  X(jes_backward, Jes)                                   \
  X(mes, Mes)                        /* mes.hip */       \
  X(mes_backward, Mes)                                   \
  X(gibbon, Gibbon)                                      \
  X(gibbon_backward, Gibbon)                             \
  X(mv_quantiles, MvQuantiles)                           \
  X(nipv_gram, Nipv)                 /* nipv.hip */      \
  X(nipv_gram_backward, Nipv)                            \
  X(bald, Bald)                      /* bald.hip */      \
  X(bald_backward, Bald)                                 \
  X(analytic, Analytic)              /* analytic.hip */  \
  X(analytic_backward, Analytic)                         \
  X(saas_potential, SaasPotential)   /* saas_nuts.hip */ \
  X(lbfgs_step, LbfgsStep)           /* lbfgs.hip */     \
  X(lbfgsb_step, Lbfgsb)             /* lbfgsb.hip */

// Every record, for bo_struct_size.
#define BO_RECORDS(X)                                                                          \
  X(PostPartials) X(QmcFinalize) X(QmcBackward) X(PostBackward) X(Qehvi) X(QehviFeas)          \
  X(Qlogehvi) X(QmcFeas) X(Kg) X(Paths) X(Jes) X(Mes) X(Gibbon) X(MvQuantiles) X(Nipv) X(Bald) \
  X(Analytic) X(SaasPotential) X(LbfgsStep) X(Lbfgsb) X(Fantasy) X(IcmCovar) X(IcmMll)          \
  X(IcmTaskView)

extern "C" {

#define BO_ENTRY(entry, record)                                         \
  int bo_##entry##_impl(const Bo##record##Args* a, void* stream);       \
  int bo_##entry##_v(const Bo##record##Args* a, void* stream) {         \
    if (!header_ok(a, "bo_" #entry "_v")) return BO_ERR_ARG;            \
    return bo_##entry##_impl(a, stream);                                \
  }
BO_RECORD_ENTRIES(BO_ENTRY)
#undef BO_ENTRY

// fantasy.hip, icm.hip: record entry points added within ABI 12.  The _v names above are
// that version's closed set, so these carry plain names; the header check is the same.
#define BO_ENTRY_PLAIN(entry, record)                                   \
  int bo_##entry##_impl(const Bo##record##Args* a, void* stream);       \
  int bo_##entry(const Bo##record##Args* a, void* stream) {             \
    if (!header_ok(a, "bo_" #entry)) return BO_ERR_ARG;                 \
    return bo_##entry##_impl(a, stream);                                \
  }
BO_ENTRY_PLAIN(fantasy_posterior, Fantasy)
BO_ENTRY_PLAIN(fantasy_posterior_backward, Fantasy)
BO_ENTRY_PLAIN(icm_covar, IcmCovar)
BO_ENTRY_PLAIN(icm_mll_terms, IcmMll)
BO_ENTRY_PLAIN(icm_task_view, IcmTaskView)
#undef BO_ENTRY_PLAIN

// sizeof of each argument record (HOST, for bindings to verify their layouts).
int64_t bo_struct_size(const char* name) {
  const std::string s = name ? name : "";
#define BO_SIZE(record) \
  if (s == "Bo" #record "Args") return sizeof(Bo##record##Args);
  BO_RECORDS(BO_SIZE)
#undef BO_SIZE
  return -1;
}

}  // extern "C"
