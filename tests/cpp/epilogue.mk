# Test infrastructure: epilogue_headers checks the epilogue overloads of include/sparsify.me/spmma.hxx against a host fp64
# evaluation.  It links the product library only (make -C tests/cpp -f epilogue.mk).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
ROOT     := ../..
CXXFLAGS ?= --offload-arch=$(ARCH) -O2 -std=c++17 -I$(ROOT)/include -Wall
LDFLAGS  := -L$(ROOT)/sparsify.me_amd -lsparsifyme -Wl,-rpath,'$$ORIGIN/../../../sparsify.me_amd'
HDRS     := $(wildcard $(ROOT)/include/sparsify.me/*.hxx $(ROOT)/include/sparsify.me/*/*.hxx $(ROOT)/include/*.h)

all: bin/epilogue_headers

bin/epilogue_headers: epilogue_headers.cpp $(HDRS) $(ROOT)/sparsify.me_amd/libsparsifyme.so
	@mkdir -p bin
	$(HIPCC) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

.PHONY: all
