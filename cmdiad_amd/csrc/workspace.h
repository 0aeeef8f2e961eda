// Caller-owned workspaces (host only, no HIP headers).  Every workspace has ONE layout function next to its launcher:
// it takes (base, problem sizes), cuts the pieces off a Carve in order and returns their typed pointers plus the total.  The
// *_workspace_bytes query is layout(nullptr, ...).total, the launcher uses the pointers of layout(workspace, ...): the size
// and the cut cannot disagree.  (A layout written as one braced return relies on the initialisers of a braced list being
// evaluated in order.)  Checked by tests/workspace_check.cpp.
#pragma once
#include <stddef.h>

#include "../../include/cmdiad_hip.h"

void cmdiad_set_error(const char* fmt, ...);

// Bump carver.  take<T>(count, pad) is the current position as a T* and moves on by count * sizeof(T) rounded up to pad bytes.
// With base == nullptr (a sizing pass) every take is nullptr and only total() means anything: the position is kept as an
// offset, and a pointer is formed from a real base only.
class Carve {
public:
    explicit Carve(void* base) : base_((char*)base) {}
    template <class T>
    T* take(size_t count, size_t pad = 1)
    {
        const size_t at = off_;
        off_ += (count * sizeof(T) + pad - 1) / pad * pad;
        return base_ ? (T*)(base_ + at) : nullptr;
    }
    size_t total() const { return off_; }

private:
    char* base_;
    size_t off_ = 0;
};

// CMDIAD_OK, or CMDIAD_ERR_WORKSPACE with the error text set: `have` bytes at `workspace` do not hold the `need` of a layout.
inline int workspace_ok(const char* who, const void* workspace, size_t have, size_t need)
{
    if (need == 0 || (workspace && have >= need)) return CMDIAD_OK;
    cmdiad_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace ? have : (size_t)0, need);   // (a null one holds 0)
    return CMDIAD_ERR_WORKSPACE;
}
