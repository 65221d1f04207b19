// Prints kb_build_layout.h's robust-mode decisions of one rig for tests/test_robust_build_mode.py:
//   test_robust_build_layout N C K wpb bpc F pipe0
//   -> for (mode, weighted) in (general, 0) (general, 1) (pipe, 0) (pipe, 1): robust_pipe robust_fits
#include <cstdio>
#include <cstdlib>

#include "../../kalibr_amd/csrc/kb_build_layout.h"

int main(int argc, char** argv) {
  if (argc != 8) {
    std::fprintf(stderr, "usage: test_robust_build_layout N C K wpb bpc F pipe0\n");
    return 2;
  }
  const kb_blay::Rig r{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                       std::atoi(argv[5])};
  const int F = std::atoi(argv[6]);
  const bool pipe0 = std::atoi(argv[7]) != 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int w = 0; w < 2; ++w)
      std::printf("%d %d ", kb_blay::robust_pipe(pipe0, mode != 0, w != 0) ? 1 : 0,
                  kb_blay::robust_fits(r, pipe0, mode != 0, w != 0, F) ? 1 : 0);
  std::printf("\n");
  return 0;
}
