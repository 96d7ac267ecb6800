// bls377_g1.hip — the G1 kernels of BLS12-377 (bucket accumulation, fold, fixed-base) in a translation unit of their own.
#include "group.cuh"
namespace zk {
ZK_INSTANTIATE_GROUP(Fe<Bls377Fq>)
ZK_INSTANTIATE_BIND(Fe<Bls377Fq>)
}  // namespace zk
