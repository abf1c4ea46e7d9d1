# Test infrastructure: linear24_headers checks spmma_plan_t<T>::linear of include/sparsify.me/spmma.hxx against the three-call route
# through the same headers.  It links the product library only (make -C tests/cpp -f linear24.mk).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
ROOT     := ../..
CXXFLAGS ?= --offload-arch=$(ARCH) -O2 -std=c++17 -I$(ROOT)/include -Wall
LDFLAGS  := -L$(ROOT)/sparsify.me_amd -lsparsifyme -Wl,-rpath,'$$ORIGIN/../../../sparsify.me_amd'
HDRS     := $(wildcard $(ROOT)/include/sparsify.me/*.hxx $(ROOT)/include/sparsify.me/*/*.hxx $(ROOT)/include/*.h)

all: bin/linear24_headers

bin/linear24_headers: linear24_headers.cpp $(HDRS) $(ROOT)/sparsify.me_amd/libsparsifyme.so
	@mkdir -p bin
	$(HIPCC) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

.PHONY: all
