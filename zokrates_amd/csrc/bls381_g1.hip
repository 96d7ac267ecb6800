// bls381_g1.hip — the G1 kernels of BLS12-381 (bucket accumulation, fold, fixed-base) in a translation unit of their own.
#include "group.cuh"
namespace zk {
ZK_INSTANTIATE_GROUP(Fe<Bls381Fq>)
ZK_INSTANTIATE_BIND(Fe<Bls381Fq>)
}  // namespace zk
// The CPU emulator build used by the tests (-DZK_EMU) compiles a fixed list of translation units that predates BLS12-377: there this
// unit carries the matching BLS12-377 one as well.  The product build compiles bls377_g1.hip on its own (zokrates_amd/build.py).
#ifdef ZK_EMU
#include "bls377_g1.hip"
#endif
