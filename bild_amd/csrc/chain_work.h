// The expected frames of a task: how many frames a candidate will run itself, estimated from its switch frames alone.
// THE definition of the rule -- the frame loop's wave priority (logl_body.h), the table walk's work-list bucket (walk_task.h),
// the device scheduler (schedule.hip: work_kernel) and the host scheduler (launch.cpp: schedule) all step this object over
// their own view of the segment list, each with its own iteration and clamping, and must agree: the one-launch path hands
// the walk's estimate to the frame loop in place of the frame loop's own.
//
// A chain = switches less than m_typ frames apart (m_typ: the transient table's typical frames-to-convergence), run as one
// piece.  A switch whose segment is at least m_typ frames long comes out of the transient table, unless a chain is in
// progress, which then ends m_typ frames behind it.  A chain of one link -- or of two, with the pair table -- is a table
// entry too and costs no frame.
#pragma once

#if defined(__HIPCC__)
#define BILD_HD __host__ __device__
#else
#define BILD_HD
#endif

namespace bild {

struct ChainWork {
    int m_typ;
    bool pairs; // the set has a pair table
    int w = 0, run_from = -1, links = 0;
    // the switch at frame t, `gap` frames in front of the next switch (or of the trajectory's end); switches in frame order
    // (on local copies: with the members updated in place three table-building kernels came out with 16 bytes more scratch)
    BILD_HD void add(int t, int gap)
    {
        int rf = run_from, lk = links, ww = w;
        if (rf < 0) {
            if (gap < m_typ) {
                rf = t;
                lk = 1;
            }
        } else {
            ++lk;
            if (gap >= m_typ) { // the chain ends m_typ frames behind this switch
                if (!(pairs && lk == 2)) ww += t + m_typ - rf;
                rf = -1;
            }
        }
        run_from = rf;
        links = lk;
        w = ww;
    }
    // behind the last switch of a trajectory of T frames: a chain that reaches the end runs to it.  Returns the estimate.
    BILD_HD int finish(int T)
    {
        if (run_from >= 0 && !(links == 1 || (pairs && links == 2))) w += T - run_from;
        return w;
    }
};

} // namespace bild
