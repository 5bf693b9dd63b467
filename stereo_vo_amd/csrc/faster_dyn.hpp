// faster_dyn.hpp -- the rule that moves dmFASTER's threshold (stage2_detect.cpp:537-546), once, for the kernels and for host code.
//
//     feats_density = nFeats / static_cast<double>(img_size.x * img_size.y);
//     if (feats_density < 0.8 * target)       m_threshold = std::max(1, m_threshold - 1);
//     else if (feats_density > 1.2 * target)  m_threshold = m_threshold + 1;
//
// nFeats is the number of ALL FAST-12 corners of one octave image (a size_t there, the full count of cand_cnt here: it counts past
// the candidate list's capacity), the arithmetic is IEEE double with one operation per operator (every unit that includes this
// header is compiled without contraction and without fast-math).  A threshold in 0 .. 255 stays there: no pixel passes I + 255, so
// at 255 nothing is a corner, the density is 0 and the rule can only step down -- or, with target = 0, stay.  T = 0 steps to 1, never
// below (max(1, -1)).
#ifndef SVO_FASTER_DYN_HPP
#define SVO_FASTER_DYN_HPP

#ifdef __HIPCC__
#define SVO_FD_FN __host__ __device__ inline
#else
#define SVO_FD_FN inline
#endif

SVO_FD_FN int faster_dyn_step(int T, unsigned n, int w, int h, double target)
{
    const double density = (double)n / (double)(w * h);
    if (density < 0.8 * target) return T - 1 > 1 ? T - 1 : 1;
    if (density > 1.2 * target) return T + 1;
    return T;
}

#undef SVO_FD_FN
#endif
