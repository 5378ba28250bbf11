// bessel_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/bessel_plan.cpp (pure host code) for tests/test_bessel_ref.py, which
// builds it with -fsanitize=address,undefined: the validation of a transform's table and the choice of q's per workgroup.  Prints one
// line per choice; exit status 0 when every validation answers as it should.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "bessel_plan.h"

using namespace dfta_bessel;

int main()
{
    int bad = 0;
    const int l[5] = {0, 1, 2, 3, 4};
    const double q[4] = {0., 1e-300, 3., 200.};
    bad += check_transform(0, 5, l, 4, q) != nullptr;
    bad += check_transform(1, 5, l, 4, q) != nullptr;
    bad += check_transform(0, 0, nullptr, 0, nullptr) != nullptr;
    bad += check_transform(2, 5, l, 4, q) == nullptr;
    bad += check_transform(-1, 5, l, 4, q) == nullptr;
    for (int wrong : {-1, 5, 100}) {
        std::vector<int> lw(l, l + 5);
        lw[3] = wrong;
        bad += check_transform(1, 5, lw.data(), 4, q) == nullptr;
    }
    for (double wrong : {-1e-300, -1., std::nan(""), std::numeric_limits<double>::infinity()}) {
        std::vector<double> qw(q, q + 4);
        qw[2] = wrong;
        bad += check_transform(0, 5, l, 4, qw.data()) == nullptr;
    }
    const double negzero[1] = {-0.};
    bad += check_transform(0, 5, l, 1, negzero) != nullptr;
    const int shapes[][2] = {{1, 256}, {3, 256}, {1000, 41}, {64, 17}, {1, 1}, {19, 17}, {2500, 1}};
    for (const auto& sh : shapes) std::printf("pick %d %d %d %d %d\n", sh[0], sh[1], 256, 0, pick_qblock(sh[0], sh[1], 256, 0));
    for (int forced : {1, 2, 4, 8, 3, 16, -1}) std::printf("pick %d %d %d %d %d\n", 1000, 41, 256, forced, pick_qblock(1000, 41, 256, forced));
    bad += num_blocks(1000, 41, 8) != 6000 || num_blocks(3, 256, 2) != 384 || num_blocks(46341, 46341, 1) != 46341L * 46341L;
    return bad;
}
