// TEST INFRASTRUCTURE ONLY: csrc/chaindp_devmem.h on its own, over a counting malloc / free that can be told to fail the k-th
// allocation.  Built with -fsanitize=address,undefined and run by tests/test_devmem_sanitizers.py; ASan's leak check at exit is part
// of the proof.  Every expectation is a CHECK: the first that fails prints its line and ends the run with a non-zero status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../minimap2_chaindp_amd/csrc/chaindp_devmem.h"

using chaindp::DevPool;
using chaindp::dev_buf;

static long g_live = 0, g_allocs = 0, g_frees = 0, g_fail_at = 0;   // g_fail_at: the k-th allocation from now fails (0: none)

static int count_alloc(void **p, size_t bytes)
{
	++g_allocs;
	if (g_fail_at > 0 && --g_fail_at == 0) return 2;
	*p = malloc(bytes);
	if (!*p) return 2;
	++g_live;
	return 0;
}

static int count_free(void *p)
{
	if (p) { --g_live; ++g_frees; }
	free(p);
	return 0;
}

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

struct Five { uint8_t *a = nullptr; int32_t *b = nullptr; const uint64_t *c = nullptr; void *d = nullptr; float *e = nullptr; };

static int five(DevPool &pool, Five &f)      // a first-use group written out: mark, the allocations, rollback on an error (what alloc_group does for chaindp_abi.cpp)
{
	const size_t m = pool.mark();
	int e = pool.alloc((void**)&f.a, 100);
	if (!e) e = pool.alloc((void**)&f.b, 0);
	if (!e) e = pool.alloc((void**)&f.c, 64);
	if (!e) e = pool.alloc(&f.d, 1);
	if (!e) e = pool.alloc((void**)&f.e, 4000);
	if (e) pool.rollback(m);
	return e;
}

static bool all_null(const Five &f) { return !f.a && !f.b && !f.c && !f.d && !f.e; }

int main()
{
	DevPool *pool = new DevPool(count_alloc, count_free);
	// alloc of 0 bytes: a non-null buffer of 8 bytes
	char *z = nullptr;
	CHECK(pool->alloc((void**)&z, 0) == 0 && z != nullptr && pool->bytes() == 8 && g_live == 1);
	memset(z, 0x5a, 8);                                               // (ASan checks the size)

	// a transaction of five allocations failing at k = 1..5 leaves nothing behind; a retry succeeds
	Five f;
	for (int k = 1; k <= 5; ++k) {
		const size_t bytes0 = pool->bytes();
		const long live0 = g_live;
		g_fail_at = k;
		CHECK(five(*pool, f) != 0);
		CHECK(all_null(f) && pool->bytes() == bytes0 && g_live == live0 && pool->mark() == 1);
		g_fail_at = 0;
	}
	CHECK(five(*pool, f) == 0 && f.a && f.b && f.c && f.d && f.e);
	CHECK(pool->bytes() == 8 + 100 + 8 + 64 + 1 + 4000 && g_live == 6);

	// the same through alloc_group, which also leaves alone a slot another group has filled
	Five g;
	CHECK(pool->alloc(&g.d, 32) == 0);
	for (int k = 1; k <= 4; ++k) {
		const size_t bytes0 = pool->bytes();
		const long live0 = g_live;
		void *const shared = g.d;
		g_fail_at = k;
		CHECK(pool->alloc_group({dev_buf(g.a, 10), dev_buf(g.b, 20), dev_buf(g.c, 30), dev_buf(g.d, 99), dev_buf(g.e, 40)}) != 0);
		CHECK(!g.a && !g.b && !g.c && !g.e && g.d == shared && pool->bytes() == bytes0 && g_live == live0);
		g_fail_at = 0;
	}
	CHECK(pool->alloc_group({dev_buf(g.a, 10), dev_buf(g.b, 20), dev_buf(g.c, 30), dev_buf(g.d, 99), dev_buf(g.e, 40)}) == 0);
	CHECK(g.a && g.b && g.c && g.e && pool->bytes() == 8 + 4173 + 32 + 100 && g_live == 11);

	// reserve, free_first = false: a failing growth leaves pointer, cap and contents; a succeeding one frees the old buffer once
	void *r = nullptr;
	size_t cap = 0;
	size_t need = 1000;
	CHECK(pool->reserve(&r, cap, need, need + need / 4, false) == 0 && r && cap == 1250);
	memset(r, 0x17, 1250);
	void *const r0 = r;
	long allocs0 = g_allocs, frees0 = g_frees;
	CHECK(pool->reserve(&r, cap, 1250, 1250 + 1250 / 4, false) == 0 && r == r0 && cap == 1250 && g_allocs == allocs0);   // need <= cap: nothing
	CHECK(pool->reserve(&r, cap, 0, 0, false) == 0 && r == r0 && cap == 1250 && g_allocs == allocs0);
	need = 2000;
	g_fail_at = 1;
	size_t bytes0 = pool->bytes();
	CHECK(pool->reserve(&r, cap, need, need + need / 4, false) != 0);
	CHECK(r == r0 && cap == 1250 && pool->bytes() == bytes0 && g_frees == frees0);
	for (int i = 0; i < 1250; ++i) CHECK(((unsigned char*)r)[i] == 0x17);
	g_fail_at = 0;
	long live0 = g_live;
	CHECK(pool->reserve(&r, cap, need, need + need / 4, false) == 0);
	CHECK(r && cap == 2500 && g_frees == frees0 + 1 && g_live == live0 && pool->bytes() == bytes0 - 1250 + 2500);
	memset(r, 0x18, 2500);

	// reserve, free_first = true: a failing growth leaves the slot null and cap 0; the next call allocates
	void *t = nullptr;
	size_t tcap = 0;
	CHECK(pool->reserve(&t, tcap, 64, 64, true) == 0 && t && tcap == 64);
	allocs0 = g_allocs;
	CHECK(pool->reserve(&t, tcap, 64, 64, true) == 0 && g_allocs == allocs0);
	bytes0 = pool->bytes(); live0 = g_live;
	g_fail_at = 1;
	CHECK(pool->reserve(&t, tcap, 65, 65 + 65 / 2 + 64, true) != 0);
	CHECK(t == nullptr && tcap == 0 && pool->bytes() == bytes0 - 64 && g_live == live0 - 1);
	g_fail_at = 0;
	CHECK(pool->reserve(&t, tcap, 65, 65 + 65 / 2 + 64, true) == 0 && t && tcap == 161 && g_live == live0);

	// the same two promises through the DevGrow overload, pointer and capacity as one value
	chaindp::DevGrow dg;
	CHECK(pool->reserve(dg, 100, 125, false) == 0 && dg.p && dg.cap == 125);
	memset(dg.p, 0x21, 125);
	void *const dg0 = dg.p;
	bytes0 = pool->bytes(); live0 = g_live; frees0 = g_frees;
	g_fail_at = 1;
	CHECK(pool->reserve(dg, 200, 250, false) != 0);
	CHECK(dg.p == dg0 && dg.cap == 125 && pool->bytes() == bytes0 && g_live == live0 && g_frees == frees0);
	for (int i = 0; i < 125; ++i) CHECK(((unsigned char*)dg.p)[i] == 0x21);
	g_fail_at = 1;
	CHECK(pool->reserve(dg, 200, 200, true) != 0);
	CHECK(dg.p == nullptr && dg.cap == 0 && pool->bytes() == bytes0 - 125 && g_live == live0 - 1);
	g_fail_at = 0;
	CHECK(pool->reserve(dg, 200, 200, true) == 0 && dg.p && dg.cap == 200 && g_live == live0 && pool->bytes() == bytes0 - 125 + 200);
	memset(dg.p, 0x22, 200);

	// release of one slot, of a slot the pool does not know
	pool->release((void**)&g.b);
	CHECK(!g.b && g_live == live0 - 1);
	void *stranger = nullptr;
	pool->release(&stranger);
	CHECK(g_live == live0 - 1);

	// release_all: nothing live, every slot null, a second call harmless
	pool->release_all();
	CHECK(g_live == 0 && pool->bytes() == 0 && pool->mark() == 0);
	CHECK(!z && all_null(f) && all_null(g) && !r && !t && !dg.p);
	pool->release_all();
	CHECK(g_live == 0 && pool->bytes() == 0);
	// ... and the pool works again afterwards; what is live when it is destroyed goes with it
	CHECK(pool->alloc(&r, 16) == 0 && g_live == 1);
	delete pool;
	CHECK(g_live == 0 && r == nullptr);
	printf("devmem ok: %ld allocations, %ld frees, live %ld\n", g_allocs, g_frees, g_live);
	return 0;
}
