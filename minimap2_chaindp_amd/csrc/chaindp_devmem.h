// chaindp_devmem.h -- the one owner of a context's device memory (host only; no HIP header: the allocator is handed in).
// A pool keeps one entry per live allocation: the address of the pointer that owns it and its size.  The pointers live in a
// heap-allocated context that never moves, so their addresses are stable; whatever frees an allocation nulls its pointer.
// The pool owns, it does not recycle: a freed buffer goes back to the allocator.  Errors are the allocator's codes, 0 = success.
#ifndef CHAINDP_DEVMEM_H
#define CHAINDP_DEVMEM_H
#include <stddef.h>
#include <initializer_list>
#include <vector>

namespace chaindp {

struct DevBuf { void **slot; size_t bytes; };
template <typename T> static inline DevBuf dev_buf(T *&p, size_t bytes) { return DevBuf{(void**)&p, bytes}; }
struct DevGrow { void *p = nullptr; size_t cap = 0; };      // a grow-only buffer and its capacity in bytes (DevPool::reserve)

class DevPool {
public:
	typedef int (*alloc_fn)(void **p, size_t bytes);
	typedef int (*free_fn)(void *p);
	DevPool(alloc_fn a, free_fn f) : alloc_(a), free_(f) {}
	DevPool(const DevPool&) = delete;
	DevPool &operator=(const DevPool&) = delete;
	~DevPool() { release_all(); }

	// fixed-size buffer into an empty slot; 0 bytes allocates 8 (no kernel argument is ever a null scratch pointer)
	int alloc(void **slot, size_t bytes)
	{
		void *q = nullptr;
		const size_t n = bytes ? bytes : 8;
		const int e = alloc_(&q, n);
		if (e) return e;
		*slot = q;
		live_.push_back(DevBuf{slot, n});
		return 0;
	}
	// Grow-only buffer: nothing happens while need <= cap; else `grown` bytes (the caller's slack formula) replace it and become cap.
	// free_first = false: the new buffer exists before the old one goes, so a failed growth leaves the old buffer and cap intact.
	// free_first = true: release, then allocate, for a lower peak (the caller has synchronised its stream); a failed growth leaves
	// the slot null and cap 0.
	int reserve(void **slot, size_t &cap, size_t need, size_t grown, bool free_first)
	{
		if (*slot && need <= cap) return 0;
		if (free_first) { release(slot); cap = 0; }
		void *q = nullptr;
		const size_t n = grown ? grown : 8;
		const int e = alloc_(&q, n);
		if (e) return e;
		DevBuf *old = find(slot);
		if (old) { (void)free_(*slot); old->bytes = n; }        // in place: marks taken before stay valid
		else live_.push_back(DevBuf{slot, n});
		*slot = q; cap = grown;
		return 0;
	}
	int reserve(DevGrow &g, size_t need, size_t grown, bool free_first) { return reserve(&g.p, g.cap, need, grown, free_first); }
	void release(void **slot)
	{
		DevBuf *b = find(slot);
		if (!b) return;
		(void)free_(*slot);
		*slot = nullptr;
		live_.erase(live_.begin() + (b - live_.data()));
	}
	// A first-use group is a transaction: m = mark(), the allocations, rollback(m) on an error (everything allocated since the mark
	// is freed and nulled, so the context is as it was and the next call tries anew), the group's ready flag last.
	size_t mark() const { return live_.size(); }
	void rollback(size_t mark)
	{
		while (live_.size() > mark) {
			(void)free_(*live_.back().slot);
			*live_.back().slot = nullptr;
			live_.pop_back();
		}
	}
	// The empty slots of a group, all of them or none (a slot that is already filled is left alone: a buffer two groups share).
	int alloc_group(std::initializer_list<DevBuf> bufs) { return alloc_group(bufs.begin(), bufs.size()); }
	int alloc_group(const DevBuf *bufs, size_t n)
	{
		const size_t m = mark();
		int e = 0;
		for (size_t k = 0; k < n && !e; ++k) if (!*bufs[k].slot) e = alloc(bufs[k].slot, bufs[k].bytes);
		if (e) rollback(m);
		return e;
	}
	void release_all() { rollback(0); }
	size_t bytes() const
	{
		size_t s = 0;
		for (const DevBuf &b : live_) s += b.bytes;
		return s;
	}

private:
	DevBuf *find(void **slot)
	{
		for (DevBuf &b : live_) if (b.slot == slot) return &b;
		return nullptr;
	}
	alloc_fn alloc_;
	free_fn free_;
	std::vector<DevBuf> live_;
};

}  // namespace chaindp
#endif
