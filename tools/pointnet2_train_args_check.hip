// Stand-alone host check of the argument handling of the interdiff_pointnet2_train_* launchers (csrc/pointnet2_bn_train.hip) under AddressSanitizer / UBSan on a CPU:
// every call below returns before it touches the device, so no GPU is needed and no sanitizer runtime is loaded into Python.  Not on the product path.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/pointnet2_train_args_check.hip interdiff_amd/csrc/pointnet2_bn_train.hip -o build_tools/pointnet2_train_args_check && build_tools/pointnet2_train_args_check
#include "../interdiff_amd/csrc/common.h"
bool g_idf_prof_on = false;
void idf_prof_mark_slow(int, hipStream_t) {}
int main() {
    alignas(256) static char ws[4096];
    float x[8] = {0};
    const size_t need = interdiff_pointnet2_train_workspace_bytes(2);
    int bad = 0;
    bad += interdiff_pointnet2_train_workspace_bytes(0) != 0 || interdiff_pointnet2_train_workspace_bytes(257) != 0 || need == 0;
    bad += interdiff_pointnet2_train_forward(nullptr, x, 2, 64, x, ws, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_forward(x, x, 0, 64, x, ws, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_forward(x, x, 257, 64, x, ws, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_forward(x, x, 2, 2049, x, ws, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_forward(x, x, 2, 64, x, ws + 4, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_forward(x, x, 2, 64, x, ws, need - 1, nullptr) != IDF_E_NOMEM;
    bad += interdiff_pointnet2_train_grads(x, x, 2, 64, nullptr, x, ws, need, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_grads(x, x, 2, 64, x, x, ws, 16, nullptr) != IDF_E_NOMEM;
    bad += interdiff_pointnet2_train_stats(ws, 2, 1.5, x, nullptr) != IDF_E_INVAL;
    bad += interdiff_pointnet2_train_stats(nullptr, 2, 0.1, x, nullptr) != IDF_E_INVAL;
    printf("argument checks failed: %d\n", bad);
    return bad;
}
