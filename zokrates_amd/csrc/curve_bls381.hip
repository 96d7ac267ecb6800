// curve_bls381.hip — instantiates the prover for BLS12-381 (/root/reference/zokrates_field/src/bls12_381.rs:1-13).
#include "core.cuh"
namespace zk {
const CurveOps* curve_ops_bls381() {
    static const CurveOps ops = make_curve_ops<CurveBls381>();
    return &ops;
}
}  // namespace zk
// The CPU emulator build used by the tests (-DZK_EMU) compiles a fixed list of translation units that predates BLS12-377: there this
// unit carries the matching BLS12-377 one as well.  The product build compiles curve_bls377.hip on its own (zokrates_amd/build.py).
#ifdef ZK_EMU
#include "curve_bls377.hip"
#endif
