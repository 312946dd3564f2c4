// sp_sparse_all.hip -- the k = 16..32 count engines, label tables, map kernels and list exports as one translation
// unit (sp_sparse2.hip uses the list bookkeeping of sp_sparse.hip).  The list filter is sp_listfilter.hip.
#include "sp_sparse.hip"
#include "sp_sparse2.hip"
