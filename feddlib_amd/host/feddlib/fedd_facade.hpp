// Host-side mirror of the reference's operator surface for the assembly + solve hot path,
// namespace FEDD, same class / method names, argument meaning and error behaviour (exceptions),
// sitting on top of the C ABI of include/fedd_hip.h.  Header-only, C++17, no Trilinos needed
// (Teuchos_shim.hpp).  Each class cites the reference declaration it mirrors.
//
//   Map                 feddlib/core/LinearAlgebra/Map_decl.hpp
//   MultiVector         feddlib/core/LinearAlgebra/MultiVector_decl.hpp
//   Matrix              feddlib/core/LinearAlgebra/Matrix_decl.hpp
//   BlockMatrix / BlockMultiVector   feddlib/core/LinearAlgebra/Block*_decl.hpp
//   Elements / FiniteElement         feddlib/core/FE/Elements.hpp, FiniteElement.hpp
//   Domain              feddlib/core/FE/Domain_decl.hpp:66-203
//   FE                  feddlib/core/FE/FE_decl.hpp:40-488
//   BCBuilder           feddlib/core/General/BCBuilder_decl.hpp:36-84
//   Problem             feddlib/problems/abstract/Problem_decl.hpp:38-229
//   Laplace / LinElas / Stokes   feddlib/problems/specific/{Laplace,LinElas,Stokes}_decl.hpp
//   MeshPartitioner     feddlib/core/Mesh/MeshPartitioner_decl.hpp (one rank: read)
//   ExporterParaView    feddlib/core/General/ExporterParaView_decl.hpp (XDMF + raw binary)
//   LinearSolver        feddlib/problems/Solver/LinearSolver_decl.hpp
//
// Differences that are deliberate: SoA mesh storage behind the same accessors; the matrix lives on
// the GPU (host copy pulled lazily by the row-view accessors); one process = one GPU = one rank.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <iostream>
#include <limits>
#include <fstream>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/fedd_hip.h"
#include "../Teuchos_shim.hpp"

typedef double default_sc;
typedef int default_lo;
typedef long long default_go;
struct default_no { };
typedef unsigned UN;

namespace FEDD {

typedef std::vector<double> vec_dbl_Type;
typedef std::vector<int> vec_int_Type;
typedef std::vector<std::vector<double>> vec2D_dbl_Type;
typedef Teuchos::RCP<vec_dbl_Type> vec_dbl_ptr_Type;
typedef Teuchos::RCP<vec_int_Type> vec_int_ptr_Type;
typedef Teuchos::RCP<vec2D_dbl_Type> vec2D_dbl_ptr_Type;
typedef std::vector<default_go> vec_GO_Type;
typedef std::vector<vec_GO_Type> vec2D_GO_Type;
typedef std::vector<vec2D_GO_Type> vec3D_GO_Type;
typedef Teuchos::RCP<vec3D_GO_Type> vec3D_GO_ptr_Type;
typedef Teuchos::RCP<Teuchos::ParameterList> ParameterListPtr_Type;
// feddlib/core/FEDDCore.hpp:115-118 (boost::function there)
typedef std::function<void(double* x, double* res, double* parameters)> RhsFunc_Type;
typedef std::function<void(double* x, double* res, double t, const double* parameters)> BC_func_Type;
typedef std::function<double(double* x, int* parameters)> CoeffFunc_Type;                      // FEDDCore.hpp:115
typedef std::function<double(double* x, double* parameters)> CoeffFuncDbl_Type;                // FEDDCore.hpp:116
// the coefficient Stokes and NavierStokes hand to FE::assemblyStress (Stokes_def.hpp:21-24, NavierStokes_def.hpp:33-36)
inline double OneFunction(double* x, int* parameter) { (void)x; (void)parameter; return 1.0; }

inline void feddCheck(int rc, const char* what) {
    TEUCHOS_TEST_FOR_EXCEPTION(rc != 0, std::runtime_error, what << ": " << fedd_last_error());
}

// One GPU context per Domain (mesh resident on the device); shared by the objects built on it.
struct DeviceContext {
    fedd_ctx* ctx = nullptr;
    long generation = 0;      // bumped by every assembly into the context
    long aleSerial = 0;       // number of the last P(w) that FE::assemblyAdditionalConvection built here (0: none)
    Teuchos::RCP<const Teuchos::Comm<int> > comm;
    explicit DeviceContext(int device) { feddCheck(fedd_ctx_create(&ctx, device, nullptr, 0, 1), "fedd_ctx_create"); }
    // One context per rank of the communicator (the reference: one MPI rank per subdomain block).  Ranks = processes:
    // GPU = LOCAL_RANK (else rank), RCCL communicator from the 128-byte id that rank 0 makes and the communicator
    // broadcasts.  Ranks = threads of one process (Teuchos::runAsRanks): one GPU, the library's host-callback transport.
    explicit DeviceContext(const Teuchos::RCP<const Teuchos::Comm<int> >& c) : comm(c) {
        const int rank = c->getRank(), size = c->getSize();
        const char* lr = std::getenv("LOCAL_RANK");
        if (size == 1) {
            feddCheck(fedd_ctx_create(&ctx, lr ? std::atoi(lr) : 0, nullptr, 0, 1), "fedd_ctx_create");
        } else if (c->backend()->inProcess()) {
            feddCheck(fedd_ctx_create(&ctx, lr ? std::atoi(lr) : 0, nullptr, rank, size), "fedd_ctx_create");
            feddCheck(fedd_comm_set_host_callbacks(ctx, &DeviceContext::exchangeCb, &DeviceContext::allreduceCb, this), "fedd_comm_set_host_callbacks");
        } else {
            unsigned char id[128] = {0};
            if (rank == 0) feddCheck(fedd_nccl_unique_id(id), "fedd_nccl_unique_id");
            c->broadcast(0, sizeof(id), id);
            feddCheck(fedd_ctx_create(&ctx, lr ? std::atoi(lr) : rank, id, rank, size), "fedd_ctx_create");
        }
    }
    // after fedd_mesh_set* and fedd_halo_set_owners: the exchange plan of the ghost imports
    void finishHaloPlan() {
        const int size = comm.is_null() ? 1 : comm->getSize();
        if (size == 1) return;
        if (!comm->backend()->inProcess()) {
            feddCheck(fedd_halo_exchange_setup(ctx), "fedd_halo_exchange_setup");
            return;
        }
        // transport-agnostic form: every rank learns what the others ask of it (an all-to-all of the gid lists, here
        // through two all-gathers: counts, then the lists padded to the longest)
        const int rank = comm->getRank();
        std::vector<int64_t> cnt(size, 0);
        feddCheck(fedd_halo_requests_sizes(ctx, cnt.data()), "fedd_halo_requests_sizes");
        int64_t mine = 0;
        for (int64_t v : cnt) mine += v;
        std::vector<int64_t> gids((size_t)std::max<int64_t>(mine, 1));
        feddCheck(fedd_halo_requests_get(ctx, gids.data()), "fedd_halo_requests_get");
        std::vector<char> allc;
        comm->gatherAll(cnt.data(), size * sizeof(int64_t), allc);
        const int64_t* ac = (const int64_t*)allc.data();          // ac[p * size + q] = what rank p asks of rank q
        int64_t longest = 1;
        for (int p = 0; p < size; ++p) {
            int64_t t = 0;
            for (int q = 0; q < size; ++q) t += ac[(size_t)p * size + q];
            longest = std::max(longest, t);
        }
        gids.resize((size_t)longest, 0);
        std::vector<char> allg;
        comm->gatherAll(gids.data(), (size_t)longest * sizeof(int64_t), allg);
        const int64_t* ag = (const int64_t*)allg.data();
        std::vector<int64_t> fromMe(size, 0), lists;
        for (int p = 0; p < size; ++p) {
            int64_t off = 0;
            for (int q = 0; q < rank; ++q) off += ac[(size_t)p * size + q];
            fromMe[p] = ac[(size_t)p * size + rank];
            lists.insert(lists.end(), ag + (size_t)p * longest + off, ag + (size_t)p * longest + off + fromMe[p]);
        }
        if (lists.empty()) lists.push_back(0);
        feddCheck(fedd_halo_requests_set(ctx, fromMe.data(), lists.data()), "fedd_halo_requests_set");
    }
    ~DeviceContext() { if (ctx) fedd_ctx_destroy(ctx); }
private:
    static int exchangeCb(void* user, int n_peers, const int32_t* peers, const int64_t* send_ptr, const double* send_buf,
                          const int64_t* recv_ptr, double* recv_buf, int dofs) {
        DeviceContext* self = (DeviceContext*)user;
        try {
            const int rank = self->comm->getRank();
            Teuchos::CommBackend* be = self->comm->backend();
            for (int k = 0; k < n_peers; ++k)
                if (send_ptr[k + 1] > send_ptr[k])
                    be->send(rank, peers[k], send_buf + send_ptr[k] * dofs, (size_t)((send_ptr[k + 1] - send_ptr[k]) * dofs));
            for (int k = 0; k < n_peers; ++k)
                if (recv_ptr[k + 1] > recv_ptr[k])
                    be->recv(peers[k], rank, recv_buf + recv_ptr[k] * dofs, (size_t)((recv_ptr[k + 1] - recv_ptr[k]) * dofs));
            return 0;
        } catch (const std::exception& e) {
            std::cerr << "facade exchange callback: " << e.what() << std::endl;
            return 1;
        }
    }
    static int allreduceCb(void* user, double* buf, int n) {
        DeviceContext* self = (DeviceContext*)user;
        try {
            self->comm->sumAll(buf, n);
            return 0;
        } catch (const std::exception& e) {
            std::cerr << "facade allreduce callback: " << e.what() << std::endl;
            return 1;
        }
    }
public:
    DeviceContext(const DeviceContext&) = delete;
    DeviceContext& operator=(const DeviceContext&) = delete;
};
typedef Teuchos::RCP<DeviceContext> DeviceContextPtr;

template <class LO = default_lo, class GO = default_go, class NO = default_no>
class Map {
public:
    typedef Teuchos::Comm<int> Comm_Type;
    typedef Teuchos::RCP<const Comm_Type> CommConstPtr_Type;
    // nGlobal = number of global ids over all ranks (-1: this rank's largest id + 1, right for one rank)
    Map(const std::vector<GO>& gids, CommConstPtr_Type comm, GO nGlobal = -1) : gids_(gids), comm_(comm) {
        for (size_t i = 0; i < gids_.size(); ++i) maxGid_ = std::max(maxGid_, gids_[i]);
        if (nGlobal >= 0) maxGid_ = nGlobal - 1;
    }
    LO getNodeNumElements() const { return (LO)gids_.size(); }
    GO getGlobalNumElements() const { return maxGid_ + 1; }
    GO getGlobalElement(LO i) const { return gids_.at(i); }
    GO getMaxAllGlobalIndex() const { return maxGid_; }
    LO getLocalElement(GO g) const {     // hash lookup, the table is built on first use
        if (lookup_.empty() && !gids_.empty()) {
            lookup_.reserve(gids_.size() * 2);
            for (size_t i = 0; i < gids_.size(); ++i) lookup_.emplace(gids_[i], (LO)i);
        }
        auto it = lookup_.find(g);
        return it == lookup_.end() ? (LO)-1 : it->second;
    }
    CommConstPtr_Type getComm() const { return comm_; }
    // vector-field map: dof = dim*node + d   (Map_def.hpp:95-107)
    Teuchos::RCP<Map> buildVecFieldMap(UN dofs) const {
        std::vector<GO> g(gids_.size() * dofs);
        for (size_t i = 0; i < gids_.size(); ++i)
            for (UN d = 0; d < dofs; ++d) g[i * dofs + d] = dofs * gids_[i] + d;
        return Teuchos::rcp(new Map(g, comm_, (GO)dofs * (maxGid_ + 1)));
    }
    const std::vector<GO>& gids() const { return gids_; }
private:
    std::vector<GO> gids_;
    mutable std::unordered_map<GO, LO> lookup_;
    GO maxGid_ = -1;
    CommConstPtr_Type comm_;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class MultiVector {
public:
    typedef Map<LO, GO, NO> Map_Type;
    typedef Teuchos::RCP<const Map_Type> MapConstPtr_Type;
    MultiVector(MapConstPtr_Type map, UN nmbVectors = 1) : map_(map), data_(nmbVectors, std::vector<SC>(map->getNodeNumElements(), 0.)) {}
    MapConstPtr_Type getMap() const { return map_; }
    UN getNumVectors() const { return (UN)data_.size(); }
    size_t getLocalLength() const { return data_[0].size(); }
    Teuchos::ArrayRCP<SC> getDataNonConst(UN i) { return Teuchos::ArrayRCP<SC>(data_.at(i).data(), data_[i].size()); }
    Teuchos::ArrayRCP<const SC> getData(UN i) const { return Teuchos::ArrayRCP<const SC>(data_.at(i).data(), data_[i].size()); }
    void putScalar(const SC& v) { for (auto& c : data_) std::fill(c.begin(), c.end(), v); }
    void update(const SC& alpha, const MultiVector& A, const SC& beta) {
        for (size_t j = 0; j < data_.size(); ++j)
            for (size_t i = 0; i < data_[j].size(); ++i) data_[j][i] = alpha * A.data_[j][i] + beta * data_[j][i];
    }
    SC norm2(UN j = 0) const {      // over all ranks (the map is a unique map: every entry counted once)
        double s = 0;
        for (SC v : data_.at(j)) s += v * v;
        if (!map_->getComm().is_null()) map_->getComm()->sumAll(&s, 1);
        return std::sqrt(s);
    }
    std::vector<SC>& raw(UN j = 0) { return data_.at(j); }
    const std::vector<SC>& raw(UN j = 0) const { return data_.at(j); }
private:
    MapConstPtr_Type map_;
    std::vector<std::vector<SC>> data_;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Matrix {
public:
    typedef Map<LO, GO, NO> Map_Type;
    typedef Teuchos::RCP<Map_Type> MapPtr_Type;
    typedef Teuchos::RCP<const Map_Type> MapConstPtr_Type;
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    // row map = unique (vec-field) map, second argument = allocation hint only (Matrix_def.hpp:46-51)
    Matrix(MapConstPtr_Type map, LO numEntries = 0) : map_(map) { (void)numEntries; }
    MapConstPtr_Type getMap(std::string = "row") const { return map_; }
    bool isFillComplete() const { return filled_; }
    void fillComplete() { filled_ = true; }
    void resumeFill() { filled_ = false; }
    // binding to the device matrix the assembly produced
    void bind(DeviceContextPtr dev, int dofs) { dev_ = dev; gen_ = dev->generation; dofs_ = dofs; hostValid_ = false; filled_ = true; }
    // block of a mixed problem held in a numbered slot beside the system matrix (fedd_matrix_store / fedd_assemble_div)
    void bindSlot(DeviceContextPtr dev, int slot) { dev_ = dev; gen_ = dev->generation; slot_ = slot; hostValid_ = false; filled_ = true; }
    int slot() const { return slot_; }
    // Matrix::scale (used by Stokes::assemble, Stokes_def.hpp:83-85)
    void scale(const SC& alpha) {
        TEUCHOS_TEST_FOR_EXCEPTION(dev_.is_null(), std::runtime_error, "Matrix::scale: no assembled data");
        feddCheck(fedd_matrix_scale(dev_->ctx, slot_, alpha), "fedd_matrix_scale");
        hostValid_ = false;
        aleScale_ *= alpha;
    }
    // provenance of a P(w) from FE::assemblyAdditionalConvection: which one of its context it is and what it was scaled by since
    void markAdditionalConvection(long serial) { aleSerial_ = serial; aleScale_ = 1.; }
    long additionalConvectionSerial() const { return aleSerial_; }
    SC additionalConvectionScale() const { return aleScale_; }
    void fillComplete(MapConstPtr_Type, MapConstPtr_Type) { filled_ = true; }
    bool isResident() const { return !dev_.is_null() && (slot_ >= 0 || gen_ == dev_->generation); }
    DeviceContextPtr device() const { return dev_; }
    void invalidateHost() { hostValid_ = false; }
    GO getGlobalNumEntries() { pull(); return (GO)val_.size(); }
    LO getNumEntriesInLocalRow(LO row) { pull(); return (LO)(rowptr_.at(row + 1) - rowptr_.at(row)); }
    // Matrix::getLocalRowView (local column indices; colGid() maps them to global dof ids)
    void getLocalRowView(LO row, Teuchos::ArrayView<const LO>& indices, Teuchos::ArrayView<const SC>& values) {
        pull();
        const int64_t b = rowptr_.at(row), e = rowptr_.at(row + 1);
        indices = Teuchos::ArrayView<const LO>(col_.data() + b, (size_t)(e - b));
        values = Teuchos::ArrayView<const SC>(val_.data() + b, (size_t)(e - b));
    }
    GO colGid(LO localCol) { pull(); return (GO)colGid_.at(localCol); }
    // y = A x on owned rows (Matrix::apply, Matrix_def.hpp:245-254)
    void apply(const MultiVector_Type& X, MultiVector_Type& Y) {
        TEUCHOS_TEST_FOR_EXCEPTION(!isResident(), std::runtime_error, "Matrix::apply: matrix is not the one resident on the device");
        feddCheck(fedd_spmv(dev_->ctx, X.raw().data(), Y.raw().data()), "fedd_spmv");
    }
    void print() {
        pull();
        for (size_t r = 0; r + 1 < rowptr_.size(); ++r)
            for (int64_t p = rowptr_[r]; p < rowptr_[r + 1]; ++p)
                std::cout << map_->getGlobalElement((LO)r) << " " << colGid_[col_[p]] << " " << val_[p] << "\n";
    }
private:
    void pull() {
        if (hostValid_) return;
        TEUCHOS_TEST_FOR_EXCEPTION(!isResident(), std::runtime_error, "Matrix: no assembled data");
        int64_t nr, nc, nnz;
        if (slot_ >= 0) {      // a stored block: local column ids of the block's own column space
            feddCheck(fedd_matrix_sizes(dev_->ctx, slot_, &nr, &nc, &nnz), "fedd_matrix_sizes");
            rowptr_.resize(nr + 1); col_.resize(nnz); val_.resize(nnz); colGid_.resize(nc);
            feddCheck(fedd_matrix_get(dev_->ctx, slot_, rowptr_.data(), col_.data(), val_.data()), "fedd_matrix_get");
            for (int64_t i = 0; i < nc; ++i) colGid_[i] = i;
            hostValid_ = true;
            return;
        }
        feddCheck(fedd_csr_sizes(dev_->ctx, &nr, &nc, &nnz), "fedd_csr_sizes");
        rowptr_.resize(nr + 1); col_.resize(nnz); val_.resize(nnz); colGid_.resize(nc);
        feddCheck(fedd_csr_get(dev_->ctx, rowptr_.data(), col_.data(), val_.data(), colGid_.data()), "fedd_csr_get");
        hostValid_ = true;
    }
    MapConstPtr_Type map_;
    DeviceContextPtr dev_;
    long gen_ = -1, aleSerial_ = 0;
    SC aleScale_ = 1.;
    int dofs_ = 1, slot_ = -1;
    bool filled_ = false, hostValid_ = false;
    std::vector<int64_t> rowptr_, colGid_;
    std::vector<int32_t> col_;
    std::vector<double> val_;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class BlockMatrix {
public:
    typedef Matrix<SC, LO, GO, NO> Matrix_Type;
    typedef Teuchos::RCP<Matrix_Type> MatrixPtr_Type;
    BlockMatrix(UN size) : n_(size), blocks_(size * size) {}
    // BlockMatrix::merge (BlockMatrix_def.hpp:119-148) happens on the device (fedd_block_merge); the flag says that the
    // device's system matrix is the merged [A B^T; B C] of this block matrix
    void setMerged(DeviceContextPtr dev) { mergedDev_ = dev; }
    DeviceContextPtr mergedDevice() const { return mergedDev_; }
    UN size() const { return n_; }
    void addBlock(const MatrixPtr_Type& m, UN i, UN j) { blocks_.at(i * n_ + j) = m; }
    bool blockExists(UN i, UN j) const { return !blocks_.at(i * n_ + j).is_null(); }
    MatrixPtr_Type getBlock(UN i, UN j) const {
        TEUCHOS_TEST_FOR_EXCEPTION(!blockExists(i, j), std::runtime_error, "Block does not exist.");
        return blocks_[i * n_ + j];
    }
private:
    UN n_;
    std::vector<MatrixPtr_Type> blocks_;
    DeviceContextPtr mergedDev_;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class BlockMultiVector {
public:
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    typedef Teuchos::RCP<MultiVector_Type> MultiVectorPtr_Type;
    BlockMultiVector(UN size) : blocks_(size) {}
    UN size() const { return (UN)blocks_.size(); }
    UN getNumVectors() const { return blocks_.empty() || blocks_[0].is_null() ? 0 : blocks_[0]->getNumVectors(); }
    void addBlock(const MultiVectorPtr_Type& mv, UN i) { blocks_.at(i) = mv; }
    Teuchos::RCP<const MultiVector_Type> getBlock(UN i) const { return blocks_.at(i); }
    MultiVectorPtr_Type getBlockNonConst(UN i) { return blocks_.at(i); }
    void putScalar(const SC& v) { for (auto& b : blocks_) if (!b.is_null()) b->putScalar(v); }
    void update(const SC& a, const BlockMultiVector& A, const SC& b) {
        for (size_t i = 0; i < blocks_.size(); ++i) blocks_[i]->update(a, *A.blocks_[i], b);
    }
private:
    std::vector<MultiVectorPtr_Type> blocks_;
};

// FiniteElement / Elements: same accessors over a flat connectivity array (FiniteElement.hpp:17-100)
class FiniteElement {
public:
    FiniteElement(const int32_t* nodes, int nen, int flag) : nodes_(nodes, nodes + nen), flag_(flag) {}
    const vec_int_Type& getVectorNodeList() const { return nodes_; }
    int getNode(int i) const { return nodes_.at(i); }
    int getFlag() const { return flag_; }
    int size() const { return (int)nodes_.size(); }
private:
    vec_int_Type nodes_;
    int flag_;
};
class Elements {
public:
    Elements(const std::vector<int32_t>& conn, int nen) : conn_(&conn), nen_(nen) {}
    UN numberElements() const { return (UN)(conn_->size() / nen_); }
    FiniteElement getElement(UN T) const { return FiniteElement(conn_->data() + (size_t)T * nen_, nen_, 0); }
    int nodesPerElement() const { return nen_; }
private:
    const std::vector<int32_t>* conn_;
    int nen_;
};
typedef Teuchos::RCP<Elements> ElementsPtr_Type;

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Domain {
public:
    typedef Map<LO, GO, NO> Map_Type;
    typedef Teuchos::RCP<const Map_Type> MapConstPtr_Type;
    typedef Teuchos::Comm<int> Comm_Type;
    typedef Teuchos::RCP<const Comm_Type> CommConstPtr_Type;

    Domain(CommConstPtr_Type comm, int dimension = 0) : comm_(comm), dim_(dimension) {}
    Domain(vec_dbl_Type coor, double l, double h, CommConstPtr_Type comm) : comm_(comm), coorRec(coor), length(l), height(h) {}
    Domain(vec_dbl_Type coor, double l, double w, double h, CommConstPtr_Type comm) : comm_(comm), coorRec(coor), length(l), width(w), height(h) {}

    // Domain::buildMesh (Domain_def.hpp:201-265): structured square / cube, P1 on any N^dim ranks, P2 on one rank
    void buildMesh(int flagsOption, std::string meshType, int dim, std::string FEType, int N, int M, int numProcsCoarseSolve = 0) {
        TEUCHOS_TEST_FOR_EXCEPTION(meshType != "Square", std::logic_error,
                                   "Select valid mesh. Structured types are 'structured' and 'structured_bfs'; only 'Square' (rectangle/box) is built here.");
        TEUCHOS_TEST_FOR_EXCEPTION(dim != 2 && dim != 3, std::logic_error, "Select valid mesh dimension. 2 or 3 dimensional meshes can be constructed.");
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P1" && FEType != "P2", std::logic_error, "Wrong FE-Type, either P1 or P2.");
        TEUCHOS_TEST_FOR_EXCEPTION(!(M >= 1), std::logic_error, "H/h is to small.");
        TEUCHOS_TEST_FOR_EXCEPTION(numProcsCoarseSolve != 0, std::logic_error, "Mpi Ranks Coarse is not supported.");
        dim_ = dim; FEType_ = FEType; n_ = N; m_ = M; flagsOption_ = flagsOption;
        const int rank = comm_->getRank(), size = comm_->getSize();
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P2" && size > 1, std::logic_error,
                                   "Domain::buildMesh: structured P2 domains are one rank in this build, the communicator has " << size);
        int nblocks = 1;
        for (int d = 0; d < dim; ++d) nblocks *= N;
        TEUCHOS_TEST_FOR_EXCEPTION(nblocks != size, std::logic_error, "Domain::buildMesh: " << N << "^" << dim << " subdomain blocks need as many ranks, the communicator has " << size);
        int dec[3] = {N, N, N}, cel[3] = {M, M, M};
        if (FEType == "P2") {
            buildStructuredP2(dec, cel, flagsOption);
            return;
        }
        // Several ranks: the rank's block (the reference's repeated map) plus four layers of ghost elements, which
        // complete the rows of the ghost nodes within three layers (row ghosts): the Schwarz boxes a rank boundary
        // crosses are then built whole on both sides and the preconditioner does not depend on the split
        const int ghosts = size > 1 ? 4 : 0;
        int64_t ne, nr, nu, ng;
        feddCheck(fedd_mesh_structured_sizes(dim, dec, cel, rank, ghosts, &ne, &nr, &nu, &ng), "fedd_mesh_structured_sizes");
        conn_.resize(ne * (dim + 1)); xyz_.resize(nr * dim); flagRep_.resize(nr); flagUni_.resize(nu);
        std::vector<int64_t> grep(nr), guni(nu), rowGhost;
        std::vector<int32_t> rowGhostFlag;
        double org[3] = {0, 0, 0}, sz[3] = {length, dim == 2 ? height : width, height};
        for (size_t d = 0; d < coorRec.size() && d < 3; ++d) org[d] = coorRec[d];
        feddCheck(fedd_mesh_structured_build(dim, dec, cel, rank, org, sz, flagsOption, ghosts, conn_.data(), xyz_.data(), grep.data(),
                                             flagRep_.data(), guni.data(), flagUni_.data()), "fedd_mesh_structured_build");
        if (ghosts >= 2) {
            int64_t nrg = 0;
            feddCheck(fedd_mesh_structured_row_ghosts(dim, dec, cel, rank, ghosts, org, sz, flagsOption, &nrg, nullptr, nullptr), "fedd_mesh_structured_row_ghosts");
            rowGhost.resize((size_t)nrg); rowGhostFlag.resize((size_t)nrg);
            if (nrg) feddCheck(fedd_mesh_structured_row_ghosts(dim, dec, cel, rank, ghosts, org, sz, flagsOption, &nrg, rowGhost.data(), rowGhostFlag.data()), "fedd_mesh_structured_row_ghosts");
        }
        finishMesh(grep, guni, dim + 1, ng, &rowGhost, &rowGhostFlag);
        // the boundary faces of the rank's mesh, flagged like the nodes strictly inside their side (include/fedd_hip.h)
        int64_t ns = 0;
        feddCheck(fedd_mesh_structured_surfaces_sizes(dim, dec, cel, rank, ghosts, &ns), "fedd_mesh_structured_surfaces_sizes");
        surf_.assign((size_t)ns * dim, 0); surfFlag_.assign((size_t)ns, 0); surfNsn_ = dim;
        feddCheck(fedd_mesh_structured_surfaces(dim, dec, cel, rank, flagsOption, ghosts, surf_.data(), surfFlag_.data()), "fedd_mesh_structured_surfaces");
        uploadSurfaces();
        if (size > 1) {     // owner of every repeated node (lowest rank whose block holds it), then the import plan
            std::vector<int32_t> owner(grep.size());
            feddCheck(fedd_mesh_structured_owner(dim, dec, cel, (int64_t)grep.size(), grep.data(), owner.data()), "fedd_mesh_structured_owner");
            feddCheck(fedd_halo_set_owners(dev_->ctx, (int64_t)grep.size(), grep.data(), owner.data()), "fedd_halo_set_owners");
            dev_->finishHaloPlan();
        }
    }
    // generic entry for externally built (e.g. unstructured, P2) meshes in the reference's data model
    void setMesh(int dim, std::string FEType, int nen, const std::vector<int32_t>& conn, const std::vector<double>& xyz,
                 const std::vector<int64_t>& gidRep, const std::vector<int64_t>& gidUni, const std::vector<int32_t>& flagUni) {
        dim_ = dim; FEType_ = FEType; conn_ = conn; xyz_ = xyz; flagUni_ = flagUni; flagRep_.assign(gidRep.size(), 0);
        int64_t ng = 0;
        for (auto g : gidRep) ng = std::max<int64_t>(ng, g + 1);
        finishMesh(gidRep, gidUni, nen, ng);
    }

    // what MeshPartitioner::readAndPartition leaves in the domain on one rank (MeshPartitioner_def.hpp:224-530,
    // MeshUnstructured::readMeshSize / readMeshEntity): INRIA .mesh file, repeated = unique = identity numbering
    // Several ranks: every rank reads the file (as in the reference), partitions the elements with the library's
    // deterministic coordinate bisection (in place of METIS_PartMeshDual, :324) -- the same partition on every rank
    // without communication -- and keeps its part plus two layers of ghost elements (row ghosts within one layer).
    void readMeshFile(const std::string& file, int dim, std::string FEType, int volumeID) {
        if (comm_->getSize() > 1) {
            readAndPartitionMeshFile(file, dim, FEType, volumeID);
            return;
        }
        int64_t nv, ne, ns;
        feddCheck(fedd_mesh_read_sizes(file.c_str(), dim, &nv, &ne, &ns), "fedd_mesh_read_sizes");
        std::vector<double> xyz(nv * dim);
        std::vector<int32_t> vflag(nv), conn(ne * (dim + 1)), eflag(ne);
        surf_.assign(ns * dim, 0); surfFlag_.assign(ns, 0);
        feddCheck(fedd_mesh_read(file.c_str(), dim, xyz.data(), vflag.data(), conn.data(), eflag.data(), surf_.data(), surfFlag_.data()), "fedd_mesh_read");
        std::vector<int64_t> gid(nv);
        for (int64_t i = 0; i < nv; ++i) gid[i] = i;
        volumeID_ = volumeID;
        setMesh(dim, FEType, dim + 1, conn, xyz, gid, gid, vflag);
        flagRep_ = vflag;
        elemFlag_ = eflag;
        surfNsn_ = dim;
        uploadSurfaces();
    }
    void readAndPartitionMeshFile(const std::string& file, int dim, std::string FEType, int volumeID) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P1", std::logic_error, "Domain::readMeshFile on several ranks: P1 meshes");
        const int rank = comm_->getRank(), size = comm_->getSize(), nen = dim + 1, layers = 2;
        int64_t nv, ne, ns;
        feddCheck(fedd_mesh_read_sizes(file.c_str(), dim, &nv, &ne, &ns), "fedd_mesh_read_sizes");
        std::vector<double> xyz(nv * dim);
        std::vector<int32_t> vflag(nv), conn(ne * nen), eflag(ne), surf(ns * dim), sflag(ns), part(ne);
        feddCheck(fedd_mesh_read(file.c_str(), dim, xyz.data(), vflag.data(), conn.data(), eflag.data(), surf.data(), sflag.data()), "fedd_mesh_read");
        feddCheck(fedd_mesh_partition(dim, nen, ne, conn.data(), nv, xyz.data(), size, part.data()), "fedd_mesh_partition");
        int64_t nel, nr, nu, nrg;
        feddCheck(fedd_mesh_partition_sizes(nen, ne, conn.data(), nv, part.data(), size, rank, layers, &nel, &nr, &nu, &nrg), "fedd_mesh_partition_sizes");
        conn_.assign(nel * nen, 0); xyz_.assign(nr * dim, 0.); flagRep_.assign(nr, 0); flagUni_.assign(nu, 0);
        std::vector<int64_t> grep(nr), guni(nu), rowGhost(nrg), egid(nel);
        std::vector<int32_t> owner(nr), rowGhostFlag(nrg);
        feddCheck(fedd_mesh_partition_extract(dim, nen, ne, conn.data(), nv, xyz.data(), vflag.data(), part.data(), size, rank, layers,
                                              conn_.data(), xyz_.data(), grep.data(), flagRep_.data(), owner.data(), guni.data(), flagUni_.data(),
                                              rowGhost.data(), rowGhostFlag.data(), egid.data()), "fedd_mesh_partition_extract");
        dim_ = dim; FEType_ = FEType; volumeID_ = volumeID;
        finishMesh(grep, guni, nen, nv, &rowGhost, &rowGhostFlag);
        // the file's surface elements whose vertices are all in the rank's repeated map, in local repeated ids
        std::vector<int32_t> repOfGlobal((size_t)nv, -1);
        for (size_t i = 0; i < grep.size(); ++i) repOfGlobal[(size_t)grep[i]] = (int32_t)i;
        surf_.clear(); surfFlag_.clear(); surfNsn_ = dim;
        for (int64_t k = 0; k < ns; ++k) {
            bool local = true;
            for (int v = 0; v < dim; ++v) local = local && repOfGlobal[(size_t)surf[k * dim + v]] >= 0;
            if (!local) continue;
            for (int v = 0; v < dim; ++v) surf_.push_back(repOfGlobal[(size_t)surf[k * dim + v]]);
            surfFlag_.push_back(sflag[k]);
        }
        uploadSurfaces();
        feddCheck(fedd_halo_set_owners(dev_->ctx, (int64_t)grep.size(), grep.data(), owner.data()), "fedd_halo_set_owners");
        dev_->finishHaloPlan();
    }
    // Domain::buildP2ofP1Domain (Domain_def.hpp -> MeshUnstructured::buildP2ofP1MeshEdge, MeshUnstructured_def.hpp:129-410)
    void buildP2ofP1Domain(const Teuchos::RCP<Domain>& domainP1) {
        TEUCHOS_TEST_FOR_EXCEPTION(comm_->getSize() > 1, std::logic_error, "Domain::buildP2ofP1Domain: one rank in this build");
        const int dim = (int)domainP1->getDimension();
        const int64_t ne = domainP1->getNumElements(), nv = domainP1->getNumPoints("Unique");
        int64_t ned = 0;
        feddCheck(fedd_mesh_p2_sizes(dim, ne, domainP1->conn_.data(), &ned), "fedd_mesh_p2_sizes");
        const int nen2 = dim == 3 ? 10 : 6;
        std::vector<int32_t> conn2(ne * nen2), flag2(nv + ned);
        std::vector<double> xyz2((nv + ned) * dim);
        feddCheck(fedd_mesh_p2_build(dim, nv, ne, domainP1->conn_.data(), domainP1->xyz_.data(), domainP1->flagRep_.data(),
                                     (int64_t)domainP1->surfFlag_.size(), domainP1->surf_.data(), domainP1->surfFlag_.data(),
                                     domainP1->volumeID_, conn2.data(), xyz2.data(), flag2.data()), "fedd_mesh_p2_build");
        std::vector<int64_t> gid(nv + ned);
        for (size_t i = 0; i < gid.size(); ++i) gid[i] = (int64_t)i;
        setMesh(dim, "P2", nen2, conn2, xyz2, gid, gid, flag2);
        flagRep_ = flag2;
        elemFlag_ = domainP1->elemFlag_;
        nP1_ = nv;
        // P2 surface elements: the vertices, then the mid nodes in the order of the line / triangle bases
        const int64_t ns = (int64_t)domainP1->surfFlag_.size();
        surfNsn_ = dim == 2 ? 3 : 6;
        surf_.assign((size_t)ns * surfNsn_, 0); surfFlag_ = domainP1->surfFlag_;
        feddCheck(fedd_mesh_p2_surfaces(dim, nv, ne, domainP1->conn_.data(), ns, domainP1->surf_.data(), surf_.data()), "fedd_mesh_p2_surfaces");
        uploadSurfaces();
    }
    // surface elements of an externally built mesh (setMesh): nsn nodes each, local repeated ids
    void setSurfaceElements(int nsn, const std::vector<int32_t>& surf, const std::vector<int32_t>& flags) {
        surfNsn_ = nsn; surf_ = surf; surfFlag_ = flags;
        uploadSurfaces();
    }
    int nodesPerSurfaceElement() const { return surfNsn_; }
    const std::vector<int32_t>& surfaceElements() const { return surf_; }
    const std::vector<int32_t>& surfaceFlags() const { return surfFlag_; }
    // element flags of a mesh read from a file on one rank (FiniteElement::getFlag); empty: no element carries a flag
    const std::vector<int32_t>& elementFlags() const { return elemFlag_; }
    int64_t numberOfP1Nodes() const { return nP1_; }      // P2-of-P1 and structured P2 domains: their first local nodes are the P1 nodes
    bool isStructuredP2() const { return structuredP2_; }

    LO getApproxEntriesPerRow() const {      // Domain_def.hpp:176-198 (allocation hint only)
        if (dim_ == 2) return FEType_ == "P1" ? 20 : 30;
        return FEType_ == "P1" ? 50 : (FEType_ == "P2" ? 80 : 100);
    }
    UN getDimension() const { return (UN)dim_; }
    std::string getFEType() const { return FEType_; }
    CommConstPtr_Type getComm() const { return comm_; }
    MapConstPtr_Type getMapUnique() const { return mapUnique_; }
    MapConstPtr_Type getMapRepeated() const { return mapRepeated_; }
    MapConstPtr_Type getMapVecFieldUnique() const { return mapUnique_->buildVecFieldMap(dim_); }
    MapConstPtr_Type getMapVecFieldRepeated() const { return mapRepeated_->buildVecFieldMap(dim_); }
    vec2D_dbl_ptr_Type getPointsRepeated() const { return points(xyz_, (size_t)mapRepeated_->getNodeNumElements(), nullptr); }
    vec2D_dbl_ptr_Type getPointsUnique() const { return points(xyz_, (size_t)mapUnique_->getNodeNumElements(), &uniOfRep_); }
    vec_int_ptr_Type getBCFlagUnique() const { return Teuchos::rcp(new vec_int_Type(flagUni_.begin(), flagUni_.end())); }
    vec_int_ptr_Type getBCFlagRepeated() const { return Teuchos::rcp(new vec_int_Type(flagRep_.begin(), flagRep_.end())); }
    ElementsPtr_Type getElementsC() const { return Teuchos::rcp(new Elements(conn_, nen_)); }
    LO getNumElements() const { return (LO)(conn_.size() / nen_); }
    GO getNumElementsGlobal() const { return (GO)(conn_.size() / nen_); }
    LO getNumPoints(std::string type = "Unique") const { return type == "Unique" ? mapUnique_->getNodeNumElements() : mapRepeated_->getNodeNumElements(); }
    void info() const {
        if (comm_->getRank() == 0)
            std::cout << "\t### Domain: dim " << dim_ << ", FE " << FEType_ << ", elements " << getNumElements() << ", nodes "
                      << mapUnique_->getGlobalNumElements() << " ###" << std::endl;
    }
    // Domain::getMesh (Domain_decl.hpp): the facade's Domain holds the mesh arrays itself, so "the mesh" is a view of it
    Teuchos::RCP<const Domain> getMesh() const { return Teuchos::RCP<const Domain>(std::shared_ptr<const Domain>(this, [](const Domain*) {})); }
    const std::vector<int32_t>& connectivity() const { return conn_; }
    // facade internals
    DeviceContextPtr device() const { return dev_; }
    // the same mesh into another context (one rank): the child contexts of the block preconditioners (LinearSolver).  The
    // context gets the REFERENCE coordinates and then the displacement in force, so that a later moveMesh means the same
    // there as on the domain's own context; the domain remembers it (weakly) for that
    void uploadMeshTo(const DeviceContextPtr& dev) const {
        std::vector<int64_t> grep(mapRepeated_->gids().begin(), mapRepeated_->gids().end()), guni(mapUnique_->gids().begin(), mapUnique_->gids().end());
        const std::vector<double>& ref = xyzRef_.empty() ? xyz_ : xyzRef_;
        feddCheck(fedd_mesh_set(dev->ctx, dim_, nen_, (int64_t)(conn_.size() / nen_), conn_.data(), (int64_t)grep.size(), ref.data(), grep.data(),
                                (int64_t)guni.size(), guni.data(), flagUni_.data()), "fedd_mesh_set");
        if (!disp_.empty()) feddCheck(fedd_mesh_move(dev->ctx, disp_.data()), "fedd_mesh_move");
        if (!dist_.empty()) feddCheck(fedd_interface_distance_set(dev->ctx, dist_.data()), "fedd_interface_distance_set");
        uploads_.push_back(dev.shared());
    }
    // Domain::moveMesh (Domain_def.hpp:673-676 -> Mesh::moveMesh, Mesh_def.hpp:297-330): points = reference points + displacement,
    // one addition per entry, relative to the points the mesh was built with (pointsRepRef_ / pointsUniRef_) and not cumulative.
    // The unique points of this facade are a view of the repeated ones (getPointsUnique), so the repeated displacement moves
    // both; the unique one is checked like the reference checks it.  The device goes first: fedd_mesh_move refuses a
    // displacement that inverts an element and then nothing, here or there, has moved.  One rank (the device call says so).
    void moveMesh(Teuchos::RCP<MultiVector<SC, LO, GO, NO> > displacementUnique, Teuchos::RCP<MultiVector<SC, LO, GO, NO> > displacementRepeated) {
        TEUCHOS_TEST_FOR_EXCEPTION(displacementRepeated.is_null(), std::runtime_error, " displacementRepeated in moveMesh is null.");
        TEUCHOS_TEST_FOR_EXCEPTION(displacementUnique.is_null(), std::runtime_error, " displacementRepeated in moveMesh is null.");
        const std::vector<SC>& d = displacementRepeated->raw(0);
        TEUCHOS_TEST_FOR_EXCEPTION(d.size() != xyz_.size(), std::runtime_error,
                                   "Domain::moveMesh: displacementRepeated has " << d.size() << " entries, the repeated points have " << xyz_.size());
        TEUCHOS_TEST_FOR_EXCEPTION(displacementUnique->raw(0).size() != (size_t)mapUnique_->getNodeNumElements() * dim_, std::runtime_error,
                                   "Domain::moveMesh: displacementUnique does not live on the unique vector-field map");
        if (xyzRef_.empty()) xyzRef_ = xyz_;       // pointsRepRef_ (and, through uniOfRep_, pointsUniRef_)
        feddCheck(fedd_mesh_move(dev_->ctx, d.data()), "fedd_mesh_move");
        for (auto& w : uploads_)
            if (auto child = w.lock()) feddCheck(fedd_mesh_move(child->ctx, d.data()), "fedd_mesh_move (child context)");
        disp_.assign(d.begin(), d.end());
        for (size_t k = 0; k < xyz_.size(); ++k) xyz_[k] = xyzRef_[k] + disp_[k];
    }
    // Domain::identifyInterfaceParallelAndDistance (Domain_def.hpp:553-566 -> MeshUnstructured::buildMeshInterfaceParallelAndDistance
    // -> MeshInterface_def.hpp:217-491): the interface of this domain is its set of nodes with one of the flags.  Per flag both
    // domains must hold the same number of such nodes (the reference's check, MeshInterface_def.hpp:254).  The two sides are
    // matched on the device (fedd_interface_match: per flag, both sides ordered lexicographically by their reference
    // coordinates and paired by rank); the tables (indicesGlobalMatched_) and the interface maps (buildInterfaceMaps) are kept.
    // This domain is the FLUID side of the device's table and domainOther the structure side, unless domainOther has already
    // identified its interface against this domain with the same flags: then that table stands and is read with the sides
    // exchanged, so that fluid->identify(structure) followed by structure->identify(fluid), as the reference's FSI main
    // calls them, leaves ONE table with the fluid as its fluid side.  A domain given as its own other side (the geometry
    // driver) has nobody to be paired with: no tables, and the getters below say so.  The distances of every repeated node to
    // the interface are computed on the device, on the points in force, and given to every context the domain is uploaded
    // to, now and at a later uploadMeshTo.  One rank (the device calls say so).
    void identifyInterfaceParallelAndDistance(Teuchos::RCP<Domain> domainOther, vec_int_Type interfaceID_vec) {
        TEUCHOS_TEST_FOR_EXCEPTION(domainOther.is_null(), std::runtime_error, "identifyInterfaceParallelAndDistance: domainOther is null.");
        for (size_t k = 0; k < interfaceID_vec.size(); ++k) {
            const int flag = interfaceID_vec[k];
            const long nThis = (long)std::count(flagUni_.begin(), flagUni_.end(), flag);
            const long nOther = (long)std::count(domainOther->flagUni_.begin(), domainOther->flagUni_.end(), flag);
            TEUCHOS_TEST_FOR_EXCEPTION(nThis != nOther, std::runtime_error,
                                       "DetermineInterfaceInParallel failed. ThisMesh and OtherMesh seem to have different numbers of interface nodes."
                                       " (flag " << flag << ": " << nThis << " against " << nOther << ")");
        }
        matchInterface(*domainOther, interfaceID_vec);
        interfaceFlags_.assign(interfaceID_vec.begin(), interfaceID_vec.end());
        haveInterfaceFlags_ = true;
        calculateDistancesToInterface();
    }
    bool hasMatchedInterface() const { return !indicesGlobalMatched_.empty(); }
    bool isFluidSideOfMatch() const { return matchThisIsFluid_; }
    // MeshInterface::getIndicesGlobalMatched (MeshInterface_def.hpp:539-553): [flag][0: this domain, 1: the other domain][j],
    // global node ids of pair j of the flag, each in its own domain's numbering.  On one rank the reference's "origin" and
    // "unique" tables are this table.
    vec3D_GO_ptr_Type getIndicesGlobalMatched() const {
        needMatch("getIndicesGlobalMatched");
        return Teuchos::rcp(new vec3D_GO_Type(indicesGlobalMatched_));
    }
    vec3D_GO_ptr_Type getIndicesGlobalMatchedOrigin() const { return getIndicesGlobalMatched(); }
    vec3D_GO_ptr_Type getIndicesGlobalMatchedUnique() const { return getIndicesGlobalMatched(); }
    // the same pairs as the device holds them: local unique node ids of this domain, the flags concatenated (interface
    // dof dim * k + c is component c of pair k); what fedd_dirichlet_nodes wants for the FaCSI rows of the fluid
    const std::vector<int32_t>& interfaceNodesLocal() const { needMatch("interfaceNodesLocal"); return interfaceLocal_; }
    // Domain::setPartialCoupling (Domain_def.hpp:766-771 -> MeshInterface::setPartialCoupling): interface nodes of this
    // flag couple only in the components the type names.  The interface maps are built again if they stand.
    void setPartialCoupling(int flag, std::string type) {
        partialCouplingFlag_.push_back(flag);
        partialCouplingType_.push_back(type);
        if (hasMatchedInterface()) buildInterfaceMaps();
    }
    // Domain::buildInterfaceMaps (Domain_def.hpp:774-876) on one rank; identifyInterfaceParallelAndDistance has called it.
    //   interface map            0 .. n-1, the interface numbering (position in the concatenated table)
    //   global interface map     this domain's global node id of every interface node, in interface order
    //   other global ...         the other domain's global node id of the same pair
    // and their vector-field maps dim * id + c.  With partial coupling the vector-field maps still list every component (the
    // uncoupled ones are the dummy dofs of assemblyDummyCoupling), the interface vector-field map is 0 .. dim n - 1, and the
    // "partial" maps list the coupled components only; the type the reference builds is "X_Y" in 3D.
    void buildInterfaceMaps() {
        needMatch("buildInterfaceMaps");
        std::vector<GO> vecGlobal, vecOther, vecInterface;
        std::vector<int> vecFlag;
        LO localID = 0;
        for (size_t i = 0; i < indicesGlobalMatched_.size(); ++i)
            for (size_t j = 0; j < indicesGlobalMatched_[i][0].size(); ++j) {
                const LO index = mapUnique_->getLocalElement(indicesGlobalMatched_[i][0][j]);
                if (index != (LO)-1) {
                    vecGlobal.push_back(indicesGlobalMatched_[i][0][j]);
                    vecOther.push_back(indicesGlobalMatched_[i][1][j]);
                    vecInterface.push_back((GO)localID);
                    vecFlag.push_back(flagUni_[(size_t)index]);
                }
                ++localID;
            }
        globalInterfaceMapUnique_ = Teuchos::rcp(new Map_Type(vecGlobal, comm_));
        interfaceMapUnique_ = Teuchos::rcp(new Map_Type(vecInterface, comm_));
        otherGlobalInterfaceMapUnique_ = Teuchos::rcp(new Map_Type(vecOther, comm_));
        partialGlobalInterfaceVecFieldMap_ = Teuchos::null;
        otherPartialGlobalInterfaceVecFieldMap_ = Teuchos::null;
        interfaceCoupled_.assign(vecGlobal.size() * (size_t)dim_, 1);
        if (partialCouplingFlag_.empty()) {
            globalInterfaceMapVecFieldUnique_ = globalInterfaceMapUnique_->buildVecFieldMap(dim_);
            interfaceMapVecFieldUnique_ = interfaceMapUnique_->buildVecFieldMap(dim_);
            otherGlobalInterfaceMapVecFieldUnique_ = otherGlobalInterfaceMapUnique_->buildVecFieldMap(dim_);
            return;
        }
        const GO numDofs = dim_;
        std::vector<GO> field, fieldPartial, otherField, otherFieldPartial, fieldInterface;
        for (size_t i = 0; i < vecGlobal.size(); ++i) {
            const int loc = isPartialCouplingFlag(vecFlag[i]);
            TEUCHOS_TEST_FOR_EXCEPTION(loc > -1 && !(partialCouplingType_[(size_t)loc] == "X_Y" && dim_ == 3), std::runtime_error,
                                       "Implement other partial coupling types.");
            for (GO dof = 0; dof < numDofs; ++dof) {
                const bool coupled = loc < 0 || dof < 2;        // "X_Y": the z component is a dummy dof
                field.push_back(numDofs * vecGlobal[i] + dof);
                otherField.push_back(numDofs * vecOther[i] + dof);
                fieldInterface.push_back((GO)fieldInterface.size());
                if (coupled) {
                    fieldPartial.push_back(numDofs * vecGlobal[i] + dof);
                    otherFieldPartial.push_back(numDofs * vecOther[i] + dof);
                }
                interfaceCoupled_[i * (size_t)dim_ + (size_t)dof] = coupled ? 1 : 0;
            }
        }
        globalInterfaceMapVecFieldUnique_ = Teuchos::rcp(new Map_Type(field, comm_));
        otherGlobalInterfaceMapVecFieldUnique_ = Teuchos::rcp(new Map_Type(otherField, comm_));
        interfaceMapVecFieldUnique_ = Teuchos::rcp(new Map_Type(fieldInterface, comm_));
        partialGlobalInterfaceVecFieldMap_ = Teuchos::rcp(new Map_Type(fieldPartial, comm_));
        otherPartialGlobalInterfaceVecFieldMap_ = Teuchos::rcp(new Map_Type(otherFieldPartial, comm_));
    }
    MapConstPtr_Type getInterfaceMapUnique() const { needMatch("getInterfaceMapUnique"); return interfaceMapUnique_; }
    MapConstPtr_Type getInterfaceMapVecFieldUnique() const { needMatch("getInterfaceMapVecFieldUnique"); return interfaceMapVecFieldUnique_; }
    MapConstPtr_Type getGlobalInterfaceMapUnique() const { needMatch("getGlobalInterfaceMapUnique"); return globalInterfaceMapUnique_; }
    MapConstPtr_Type getGlobalInterfaceMapVecFieldUnique() const { needMatch("getGlobalInterfaceMapVecFieldUnique"); return globalInterfaceMapVecFieldUnique_; }
    MapConstPtr_Type getOtherGlobalInterfaceMapUnique() const { needMatch("getOtherGlobalInterfaceMapUnique"); return otherGlobalInterfaceMapUnique_; }
    MapConstPtr_Type getOtherGlobalInterfaceMapVecFieldUnique() const { needMatch("getOtherGlobalInterfaceMapVecFieldUnique"); return otherGlobalInterfaceMapVecFieldUnique_; }
    // null without partial coupling, as in the reference (FSI::assemble asks is_null())
    MapConstPtr_Type getGlobalInterfaceMapVecFieldPartial() const { return partialGlobalInterfaceVecFieldMap_; }
    MapConstPtr_Type getOtherGlobalInterfaceMapVecFieldPartial() const { return otherPartialGlobalInterfaceVecFieldMap_; }
    // one byte per interface dof, 0 = a dummy dof of the partial coupling: the coupled_mask of fedd_fsi_merge
    const std::vector<uint8_t>& interfaceCoupledMask() const { needMatch("interfaceCoupledMask"); return interfaceCoupled_; }
    // Domain::calculateDistancesToInterface (Domain_def.hpp:568-648) with the flags of the last identify call
    void calculateDistancesToInterface() {
        TEUCHOS_TEST_FOR_EXCEPTION(!haveInterfaceFlags_, std::runtime_error,
                                   "Domain::calculateDistancesToInterface: no interface; call identifyInterfaceParallelAndDistance first");
        int64_t nInterface = 0;
        feddCheck(fedd_interface_distance(dev_->ctx, (int)interfaceFlags_.size(), interfaceFlags_.data(), &nInterface), "fedd_interface_distance");
        dist_.assign((size_t)mapRepeated_->getNodeNumElements(), 0.);
        feddCheck(fedd_interface_distance_get(dev_->ctx, dist_.data()), "fedd_interface_distance_get");
        distributeDistances();
    }
    // on the repeated map, in this facade's local order (the order of getPointsRepeated)
    vec_dbl_ptr_Type getDistancesToInterface() const {
        TEUCHOS_TEST_FOR_EXCEPTION(dist_.empty(), std::runtime_error, "Domain::getDistancesToInterface: no distances; call identifyInterfaceParallelAndDistance first");
        return Teuchos::rcp(new vec_dbl_Type(dist_.begin(), dist_.end()));
    }
    void setDistancesToInterface(vec_dbl_ptr_Type dist) {
        TEUCHOS_TEST_FOR_EXCEPTION(dist.is_null() || dist->size() != (size_t)mapRepeated_->getNodeNumElements(), std::runtime_error,
                                   "Domain::setDistancesToInterface: the distances do not live on the repeated map");
        dist_.assign(dist->begin(), dist->end());
        feddCheck(fedd_interface_distance_set(dev_->ctx, dist_.data()), "fedd_interface_distance_set");
        distributeDistances();
    }
    bool hasDistancesToInterface() const { return !dist_.empty(); }
    vec2D_dbl_ptr_Type getPointsRepeatedRef() const { return points(xyzRef_.empty() ? xyz_ : xyzRef_, (size_t)mapRepeated_->getNodeNumElements(), nullptr); }
    vec2D_dbl_ptr_Type getPointsUniqueRef() const { return points(xyzRef_.empty() ? xyz_ : xyzRef_, (size_t)mapUnique_->getNodeNumElements(), &uniOfRep_); }
    int nodesPerElement() const { return nen_; }
    const std::vector<double>& xyzRepeated() const { return xyz_; }
    const std::vector<int32_t>& uniqueLocalOfRepeated() const { return uniOfRep_; }
    // several ranks: nodes of other ranks whose rows this rank also builds (fedd_mesh_set_rows); their device node id is
    // number of unique nodes + position here
    const std::vector<int32_t>& rowGhostRepeatedIds() const { return rowGhostRep_; }
    const std::vector<int32_t>& rowGhostFlags() const { return rowGhostFlag_; }

private:
    // The reference's structured P2 lattice (MeshStructured_def.hpp:468-619, 808-994; fedd_mesh_structured_p2_build) on one rank.
    // The maps carry the reference's global ids; the LOCAL order of nodes, vectors and matrices is vertices first
    // (fedd_mesh_p2_vertices_first): local node k < numberOfP1Nodes() is node k of the structured P1 domain of the same N, M,
    // which is what the device layer's "pressure = the first nodes" convention needs.  Local id -> reference id is
    // getMapRepeated()->getGlobalElement(); the exporter writes at global positions, so its files are in reference numbering.
    void buildStructuredP2(const int* dec, const int* cel, int flagsOption) {
        const int dim = dim_;
        bool unit = length == 1. && height == 1. && (dim == 2 || width == 1.);
        for (size_t d = 0; d < coorRec.size() && d < (size_t)dim; ++d) unit = unit && coorRec[d] == 0.;
        TEUCHOS_TEST_FOR_EXCEPTION(!unit, std::logic_error, "Domain::buildMesh: structured P2 meshes are built on the unit square / cube");
        int64_t nr, nu, ne, np1;
        feddCheck(fedd_mesh_structured_p2_sizes(dim, dec, cel, 0, &nr, &nu, &ne), "fedd_mesh_structured_p2_sizes");
        const int nen = dim == 3 ? 10 : 6;
        std::vector<double> xyz(nr * dim);
        std::vector<int64_t> gref(nr), guniRef(nu);
        std::vector<int32_t> frep(nr), funi(nu), conn(ne * nen), perm(nr), inv(nr);
        feddCheck(fedd_mesh_structured_p2_build(dim, dec, cel, 0, flagsOption, xyz.data(), gref.data(), guniRef.data(), nullptr, frep.data(),
                                                funi.data(), conn.data(), nullptr), "fedd_mesh_structured_p2_build");
        feddCheck(fedd_mesh_p2_vertices_first(dim, dec, cel, 0, perm.data(), &np1), "fedd_mesh_p2_vertices_first");
        for (int64_t i = 0; i < nr; ++i) inv[perm[i]] = (int32_t)i;
        // one rank: unique = repeated, in the same order
        conn_.resize(conn.size()); xyz_.resize(xyz.size()); flagRep_.resize(nr); flagUni_.resize(nr);
        std::vector<int64_t> grep(nr);
        for (size_t k = 0; k < conn.size(); ++k) conn_[k] = inv[conn[k]];
        for (int64_t i = 0; i < nr; ++i) {
            for (int d = 0; d < dim; ++d) xyz_[i * dim + d] = xyz[(int64_t)perm[i] * dim + d];
            flagRep_[i] = frep[perm[i]];
            flagUni_[i] = funi[perm[i]];
            grep[i] = gref[perm[i]];
        }
        nP1_ = np1;
        structuredP2_ = true;
        finishMesh(grep, grep, nen, nr);
        // boundary faces: those of the P1 mesh (whose ids are the first local ids here), then the mid nodes in the slot order of
        // fedd_mesh_p2_surfaces: P1 node (r,s,t) is lattice node (2r,2s,2t), a mid node lies half-way in lattice indices
        int64_t ns = 0;
        feddCheck(fedd_mesh_structured_surfaces_sizes(dim, dec, cel, 0, 0, &ns), "fedd_mesh_structured_surfaces_sizes");
        std::vector<int32_t> s1((size_t)ns * dim);
        surfFlag_.assign((size_t)ns, 0);
        feddCheck(fedd_mesh_structured_surfaces(dim, dec, cel, 0, flagsOption, 0, s1.data(), surfFlag_.data()), "fedd_mesh_structured_surfaces");
        surfNsn_ = dim == 2 ? 3 : 6;
        surf_.assign((size_t)ns * surfNsn_, 0);
        const int64_t n1[3] = {cel[0] + 1, cel[1] + 1, dim == 3 ? cel[2] + 1 : 1}, p2m[2] = {2 * cel[0] + 1, 2 * cel[1] + 1};
        const int pairs[3][2] = {{0, 1}, {1, 2}, {0, 2}};
        for (int64_t k = 0; k < ns; ++k) {
            int64_t ref[3];
            for (int v = 0; v < dim; ++v) {
                const int64_t id = s1[k * dim + v], r = id % n1[0], s = (id / n1[0]) % n1[1], t = id / (n1[0] * n1[1]);
                ref[v] = 2 * r + p2m[0] * (2 * s + p2m[1] * 2 * t);
                surf_[k * surfNsn_ + v] = inv[ref[v]];
            }
            for (int m = 0; m < surfNsn_ - dim; ++m) surf_[k * surfNsn_ + dim + m] = inv[(ref[pairs[m][0]] + ref[pairs[m][1]]) / 2];
        }
        uploadSurfaces();
    }
    void finishMesh(const std::vector<int64_t>& grep, const std::vector<int64_t>& guni, int nen, int64_t nGlobal,
                    const std::vector<int64_t>* rowGhost = nullptr, const std::vector<int32_t>* rowGhostFlag = nullptr) {
        nen_ = nen;
        std::vector<GO> gr(grep.begin(), grep.end()), gu(guni.begin(), guni.end());
        mapRepeated_ = Teuchos::rcp(new Map_Type(gr, comm_, (GO)nGlobal));
        mapUnique_ = Teuchos::rcp(new Map_Type(gu, comm_, (GO)nGlobal));
        // repeated-local id of every unique node (for getPointsUnique)
        uniOfRep_.assign(guni.size(), -1);
        std::vector<std::pair<int64_t, int32_t>> s(grep.size());
        for (size_t i = 0; i < grep.size(); ++i) s[i] = {grep[i], (int32_t)i};
        std::sort(s.begin(), s.end());
        for (size_t i = 0; i < guni.size(); ++i) {
            auto it = std::lower_bound(s.begin(), s.end(), std::make_pair(guni[i], (int32_t)-1));
            TEUCHOS_TEST_FOR_EXCEPTION(it == s.end() || it->first != guni[i], std::runtime_error, "unique node missing from repeated map");
            uniOfRep_[i] = it->second;
        }
        dev_ = Teuchos::rcp(new DeviceContext(comm_));
        clearMatch();       // (a new mesh: the device has released the table with the old context)
        rowGhostRep_.clear();
        rowGhostFlag_.clear();
        if (rowGhost) {     // their repeated-local ids (coordinates) and flags: the Dirichlet treatment covers their rows too
            for (size_t k = 0; k < rowGhost->size(); ++k) {
                auto it = std::lower_bound(s.begin(), s.end(), std::make_pair((*rowGhost)[k], (int32_t)-1));
                TEUCHOS_TEST_FOR_EXCEPTION(it == s.end() || it->first != (*rowGhost)[k], std::runtime_error, "row ghost missing from repeated map");
                rowGhostRep_.push_back(it->second);
                rowGhostFlag_.push_back((*rowGhostFlag)[k]);
            }
        }
        if (rowGhost && !rowGhost->empty())
            feddCheck(fedd_mesh_set_rows(dev_->ctx, dim_, nen_, (int64_t)(conn_.size() / nen_), conn_.data(), (int64_t)grep.size(), xyz_.data(),
                                         grep.data(), (int64_t)guni.size(), guni.data(), flagUni_.data(), (int64_t)rowGhost->size(),
                                         rowGhost->data(), rowGhostFlag->data()), "fedd_mesh_set_rows");
        else
            feddCheck(fedd_mesh_set(dev_->ctx, dim_, nen_, (int64_t)(conn_.size() / nen_), conn_.data(), (int64_t)grep.size(), xyz_.data(),
                                    grep.data(), (int64_t)guni.size(), guni.data(), flagUni_.data()), "fedd_mesh_set");
    }
    void needMatch(const char* who) const {
        TEUCHOS_TEST_FOR_EXCEPTION(indicesGlobalMatched_.empty(), std::runtime_error,
                                   "Domain::" << who << ": no matched interface; call identifyInterfaceParallelAndDistance with the other "
                                   "domain first (a domain given as its own other side is not matched)");
    }
    int isPartialCouplingFlag(int flag) const {      // MeshInterface::isPartialCouplingFlag: the position, or -1
        auto it = std::find(partialCouplingFlag_.begin(), partialCouplingFlag_.end(), flag);
        return it == partialCouplingFlag_.end() ? -1 : (int)std::distance(partialCouplingFlag_.begin(), it);
    }
    void clearMatch() {
        indicesGlobalMatched_.clear();
        interfaceLocal_.clear();
        interfaceCoupled_.clear();
        matchFlags_.clear();
        matchPartner_.reset();
        matchThisIsFluid_ = false;
        interfaceMapUnique_ = interfaceMapVecFieldUnique_ = globalInterfaceMapUnique_ = globalInterfaceMapVecFieldUnique_ = Teuchos::null;
        otherGlobalInterfaceMapUnique_ = otherGlobalInterfaceMapVecFieldUnique_ = Teuchos::null;
        partialGlobalInterfaceVecFieldMap_ = otherPartialGlobalInterfaceVecFieldMap_ = Teuchos::null;
    }
    // the device's table between this domain's context and the other's, into indicesGlobalMatched_ and the maps
    void matchInterface(Domain& other, const vec_int_Type& interfaceID_vec) {
        if (&other == this) {
            clearMatch();
            return;
        }
        fedd_ctx *mine = dev_->ctx, *theirs = other.dev_->ctx;
        const std::vector<int32_t> flags(interfaceID_vec.begin(), interfaceID_vec.end());
        int haveMine = 0, haveTheirs = 0;
        feddCheck(fedd_interface_match_info(mine, &haveMine, nullptr, nullptr, nullptr), "fedd_interface_match_info");
        feddCheck(fedd_interface_match_info(theirs, &haveTheirs, nullptr, nullptr, nullptr), "fedd_interface_match_info");
        // the other domain matched itself (as the fluid side) against this one with these flags, and both contexts still hold it
        const bool stands = haveMine && haveTheirs && other.matchThisIsFluid_ && other.matchFlags_ == flags &&
                            other.matchPartner_.lock().get() == dev_.get() && other.hasMatchedInterface();
        clearMatch();
        if (!stands) feddCheck(fedd_interface_match(mine, theirs, (int)flags.size(), flags.data()), "fedd_interface_match");
        int64_t nPairs = 0;
        int nFlags = 0;
        feddCheck(fedd_interface_match_sizes(mine, &nPairs, &nFlags, nullptr), "fedd_interface_match_sizes");
        TEUCHOS_TEST_FOR_EXCEPTION(nFlags != (int)flags.size(), std::logic_error, "identifyInterfaceParallelAndDistance: the device's table has other flags");
        std::vector<int32_t> idFluid((size_t)nPairs), idStructure((size_t)nPairs);
        std::vector<int64_t> ptr((size_t)nFlags + 1);
        feddCheck(fedd_interface_match_get(mine, idFluid.data(), idStructure.data(), ptr.data()), "fedd_interface_match_get");
        const std::vector<int32_t>& idThis = stands ? idStructure : idFluid;
        const std::vector<int32_t>& idOther = stands ? idFluid : idStructure;
        indicesGlobalMatched_.assign((size_t)nFlags, vec2D_GO_Type(2));
        for (int q = 0; q < nFlags; ++q)
            for (int64_t k = ptr[(size_t)q]; k < ptr[(size_t)q + 1]; ++k) {     // device node id = local id of the unique map
                indicesGlobalMatched_[(size_t)q][0].push_back(mapUnique_->getGlobalElement((LO)idThis[(size_t)k]));
                indicesGlobalMatched_[(size_t)q][1].push_back(other.mapUnique_->getGlobalElement((LO)idOther[(size_t)k]));
            }
        interfaceLocal_ = idThis;
        matchFlags_ = flags;
        matchPartner_ = other.dev_.shared();
        matchThisIsFluid_ = !stands;
        buildInterfaceMaps();
    }
    void distributeDistances() {     // to the contexts of uploadMeshTo, as moveMesh does for the displacement
        for (auto& w : uploads_)
            if (auto child = w.lock()) feddCheck(fedd_interface_distance_set(child->ctx, dist_.data()), "fedd_interface_distance_set (child context)");
    }
    void uploadSurfaces() {      // with the mesh: the boundary elements the surface load vectors integrate over
        feddCheck(fedd_surface_set(dev_->ctx, surfNsn_, (int64_t)surfFlag_.size(), surf_.data(), surfFlag_.data()), "fedd_surface_set");
    }
    vec2D_dbl_ptr_Type points(const std::vector<double>& xyz, size_t n, const std::vector<int32_t>* idx) const {
        vec2D_dbl_ptr_Type p = Teuchos::rcp(new vec2D_dbl_Type(n, vec_dbl_Type(dim_, 0.)));
        for (size_t i = 0; i < n; ++i) {
            const size_t src = idx ? (size_t)(*idx)[i] : i;
            for (int d = 0; d < dim_; ++d) (*p)[i][d] = xyz[src * dim_ + d];
        }
        return p;
    }
    CommConstPtr_Type comm_;
    vec_dbl_Type coorRec;
    double length = 1., width = 1., height = 1.;
    int dim_ = 0, n_ = 0, m_ = 0, flagsOption_ = 0, nen_ = 0, surfNsn_ = 0;
    std::string FEType_;
    std::vector<int32_t> conn_, flagRep_, flagUni_, uniOfRep_, surf_, surfFlag_, rowGhostRep_, rowGhostFlag_, elemFlag_;
    std::vector<double> xyz_;
    std::vector<double> dist_;                  // distances to the interface on the repeated map (empty: none)
    std::vector<int32_t> interfaceFlags_;       // the flags of the last identifyInterfaceParallelAndDistance
    bool haveInterfaceFlags_ = false;
    // the matched interface (identifyInterfaceParallelAndDistance against another domain; empty: none)
    vec3D_GO_Type indicesGlobalMatched_;        // [flag][0: this, 1: other][j] global node ids
    std::vector<int32_t> interfaceLocal_;       // this side of the device's table: local unique node ids, flags concatenated
    std::vector<int32_t> matchFlags_;
    std::weak_ptr<DeviceContext> matchPartner_; // the other domain's context at the time of the match
    bool matchThisIsFluid_ = false;             // this domain's context is the fluid side of the device's table
    vec_int_Type partialCouplingFlag_;
    std::vector<std::string> partialCouplingType_;
    std::vector<uint8_t> interfaceCoupled_;
    Teuchos::RCP<Map_Type> interfaceMapUnique_, interfaceMapVecFieldUnique_, globalInterfaceMapUnique_, globalInterfaceMapVecFieldUnique_,
        otherGlobalInterfaceMapUnique_, otherGlobalInterfaceMapVecFieldUnique_, partialGlobalInterfaceVecFieldMap_,
        otherPartialGlobalInterfaceVecFieldMap_;
    std::vector<double> xyzRef_, disp_;         // moveMesh: the points the mesh was built with, the displacement in force (empty: never moved)
    mutable std::vector<std::weak_ptr<DeviceContext> > uploads_;     // contexts of uploadMeshTo
    int volumeID_ = 10;
    int64_t nP1_ = 0;
    bool structuredP2_ = false;
    Teuchos::RCP<Map_Type> mapRepeated_, mapUnique_;
    DeviceContextPtr dev_;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class FE {
public:
    typedef Domain<SC, LO, GO, NO> Domain_Type;
    typedef Teuchos::RCP<const Domain_Type> DomainConstPtr_Type;
    typedef Matrix<SC, LO, GO, NO> Matrix_Type;
    typedef Teuchos::RCP<Matrix_Type> MatrixPtr_Type;
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    typedef Teuchos::RCP<MultiVector_Type> MultiVectorPtr_Type;

    FE(bool saveAssembly = false) { (void)saveAssembly; }
    void addFE(DomainConstPtr_Type domain) { domainVec_.push_back(domain); }
    void doSetZeros(double eps = 10 * 2.220446049250313e-16) { setZeros_ = true; myeps_ = eps; }

    // FE_def.hpp:6932-6953
    UN checkFE(int dim, std::string FEType) const {
        for (UN i = 0; i < domainVec_.size(); ++i)
            if ((int)domainVec_[i]->getDimension() == dim && domainVec_[i]->getFEType() == FEType) return i;
        TEUCHOS_TEST_FOR_EXCEPTION(true, std::runtime_error, "Wrong FEType or dimension. No assembly possible.");
        return 0;
    }
    void assemblyLaplace(int dim, std::string FEType, int degree, MatrixPtr_Type& A, bool callFillComplete = true, int FELocExternal = -1) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        (void)degree;
        assembleInto(FELocExternal < 0 ? checkFE(dim, FEType) : (UN)FELocExternal, 1, FEDD_BLOCK_SCALAR, FEDD_FORM_LAPLACE, nullptr, A, callFillComplete);
    }
    void assemblyLaplaceVecField(int dim, std::string FEType, int degree, MatrixPtr_Type& A, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P1-disc" || FEType == "P0", std::logic_error, "Not implemented for P0 or P1-disc");
        (void)degree;
        // doSetZeros (FE_def.hpp:74-79, 719-721): element contributions below myeps_ are dropped before they are added
        feddCheck(fedd_set_option(domainVec_.at(checkFE(dim, FEType))->device()->ctx, "asm_zero_eps", setZeros_ ? myeps_ : 0.), "fedd_set_option");
        assembleInto(checkFE(dim, FEType), dim, FEDD_BLOCK_DIAG, FEDD_FORM_LAPLACE_VEC, nullptr, A, callFillComplete);
    }
    void assemblyMass(int dim, std::string FEType, std::string fieldType, MatrixPtr_Type& A, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        if (fieldType == "Scalar") assembleInto(checkFE(dim, FEType), 1, FEDD_BLOCK_SCALAR, FEDD_FORM_MASS, nullptr, A, callFillComplete);
        else if (fieldType == "Vector") assembleInto(checkFE(dim, FEType), dim, FEDD_BLOCK_DIAG, FEDD_FORM_MASS_VEC, nullptr, A, callFillComplete);
        else TEUCHOS_TEST_FOR_EXCEPTION(true, std::logic_error, "Specify valid vieldType for assembly of mass matrix.");
    }
    // FE::assemblyBDStabilization (FE_def.hpp:2151-2220): the Bochev-Dohrmann pressure block of P1/P1 Stokes
    void assemblyBDStabilization(int dim, std::string FEType, MatrixPtr_Type& A, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P1", std::logic_error, "Only implemented for P1. Q1 is equivalent but we need to adjust scaling for the reference element.");
        assembleInto(checkFE(dim, FEType), 1, FEDD_BLOCK_SCALAR, FEDD_FORM_BDSTAB, nullptr, A, callFillComplete);
    }
    void assemblyLinElasXDim(int dim, std::string FEType, MatrixPtr_Type& A, double lambda, double mu, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        const double p[2] = {lambda, mu};
        assembleInto(checkFE(dim, FEType), dim, FEDD_BLOCK_FULL, FEDD_FORM_LINELAS, p, A, callFillComplete);
    }
    // FE::assemblyLaplaceXDim (FE_def.hpp:2225-2402): the vector Laplacian with func(mean distance of the element's vertices to the
    // interface) per element, on the DIAG pattern, no doSetZeros.  The device applies HeuristicScaling (Geometry_def.hpp:24-34)
    // itself from parameters = {distance, coefficient}; func is therefore CHECKED, not used: it must return parameters[1] below
    // parameters[0] and 1.0 at and above it.  Another function is refused with what is built.
    void assemblyLaplaceXDim(int dim, std::string FEType, MatrixPtr_Type& A, CoeffFuncDbl_Type func, double* parameters, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        TEUCHOS_TEST_FOR_EXCEPTION(!func || !parameters, std::runtime_error, "assemblyLaplaceXDim: func or parameters is null.");
        auto dom = domainVec_.at(checkFE(dim, FEType));
        TEUCHOS_TEST_FOR_EXCEPTION(!dom->hasDistancesToInterface(), std::logic_error,
                                   "assemblyLaplaceXDim needs the distances to the interface: call Domain::identifyInterfaceParallelAndDistance first");
        const double dist = parameters[0], coeff = parameters[1];
        const double below = std::nextafter(dist, -std::numeric_limits<double>::infinity()), above = std::nextafter(dist, std::numeric_limits<double>::infinity());
        double probes[5] = {below, 0.5 * dist, dist, above, 2. * dist + 1.};
        bool same = true;
        for (int k = 0; k < 5; ++k) {
            double x[1] = {probes[k]};
            const double want = x[0] < dist ? coeff : 1.0;
            const double got = func(x, parameters);
            same = same && got == want;
        }
        TEUCHOS_TEST_FOR_EXCEPTION(!same, std::logic_error,
                                   "assemblyLaplaceXDim: func is not HeuristicScaling (parameters[1] where x[0] < parameters[0], else 1.0); what is built is "
                                   "the scaled Laplacian with that function, which the device evaluates itself from parameters = {distance, coefficient}");
        assembleInto(checkFE(dim, FEType), dim, FEDD_BLOCK_DIAG, FEDD_FORM_LAPLACE_XDIM, parameters, A, callFillComplete);
    }
    // FE::assemblyStress (FE_def.hpp:2407-2733): int func(x) grad v : (grad u + grad u^T), the velocity block in stress form, on
    // the FULL pattern.  func is evaluated on the host at x_k = B xi_k + p_1 of every element and quadrature point of the rule
    // determineDegree(dim, FEType, FEType, Grad, Grad) (:2427, 2487-2493, 2616-2625) and handed to the device as an array; the
    // facade's OneFunction needs no array.
    void assemblyStress(int dim, std::string FEType, MatrixPtr_Type& A, CoeffFunc_Type func, int* parameters, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        TEUCHOS_TEST_FOR_EXCEPTION(A.is_null(), std::runtime_error, "Matrix is null.");
        auto dom = domainVec_.at(checkFE(dim, FEType));
        TEUCHOS_TEST_FOR_EXCEPTION((size_t)A->getMap()->getNodeNumElements() != (size_t)dom->getMapUnique()->getNodeNumElements() * dim,
                                   std::logic_error, "Matrix row map does not match the unique map of the domain.");
        typedef double (*plain_fn)(double*, int*);
        const plain_fn* target = func.template target<plain_fn>();
        const bool one = target && *target == static_cast<plain_fn>(&OneFunction);
        std::vector<double> cq;
        if (!one) {
            const int nen = dom->nodesPerElement(), deg = nen == dim + 1 ? 1 : 2;
            int nq = 0;
            feddCheck(fedd_fe_quadrature(dim, deg, &nq, nullptr, nullptr), "fedd_fe_quadrature");
            std::vector<double> xi((size_t)nq * dim), w((size_t)nq);
            feddCheck(fedd_fe_quadrature(dim, deg, &nq, xi.data(), w.data()), "fedd_fe_quadrature");
            const auto& conn = dom->connectivity();
            const auto& xyz = dom->xyzRepeated();
            const size_t nel = conn.size() / nen;
            cq.resize(nel * nq);
            std::vector<double> x(dim);
            for (size_t T = 0; T < nel; ++T) {
                const double* p1 = &xyz[(size_t)conn[T * nen] * dim];
                for (int k = 0; k < nq; ++k) {
                    for (int d = 0; d < dim; ++d) {
                        x[d] = 0.;
                        for (int r = 0; r < dim; ++r) x[d] += (xyz[(size_t)conn[T * nen + r + 1] * dim + d] - p1[d]) * xi[(size_t)k * dim + r];
                        x[d] += p1[d];
                    }
                    cq[T * nq + k] = func(x.data(), parameters);
                }
            }
        }
        fedd_ctx* ctx = dom->device()->ctx;
        int64_t nnz;
        feddCheck(fedd_pattern_build(ctx, dim, FEDD_BLOCK_FULL, &nnz), "fedd_pattern_build");
        feddCheck(fedd_assemble_stress(ctx, one ? nullptr : cq.data(), (int64_t)cq.size()), "fedd_assemble_stress");
        dom->device()->generation++;
        A->bind(dom->device(), dim);
        if (!callFillComplete) A->resumeFill();
    }
    // FE::assemblyAdditionalConvection (FE_def.hpp:3044-3255): P(w) for the mesh velocity w on the repeated vector-field map.  w is
    // uploaded (fedd_mesh_velocity_set), FEDD_ALE_P runs into slot 3 -- the slot of the stabilisation block C, which a P2 / P1
    // problem leaves free; P1 velocities are refused for that reason -- and the matrix returned is bound to it, with the positive
    // sign of the reference.  The matrix remembers that it is the last P of its context (NavierStokes::reAssembleFSI checks).
    void assemblyAdditionalConvection(int dim, std::string FEType, MatrixPtr_Type& A, MultiVectorPtr_Type w, bool callFillComplete = true) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P2", std::logic_error,
                                   "assemblyAdditionalConvection: built for P2 velocities (P lives in slot 3, which holds C for P1 / P1)");
        TEUCHOS_TEST_FOR_EXCEPTION(A.is_null() || w.is_null(), std::runtime_error, "Matrix or mesh velocity is null.");
        auto dom = domainVec_.at(checkFE(dim, FEType));
        TEUCHOS_TEST_FOR_EXCEPTION(w->raw(0).size() != (size_t)dom->getMapRepeated()->getNodeNumElements() * dim, std::logic_error,
                                   "assemblyAdditionalConvection: w does not live on the repeated vector-field map of the domain");
        auto dev = dom->device();
        feddCheck(fedd_mesh_velocity_set(dev->ctx, w->raw(0).data()), "fedd_mesh_velocity_set");
        feddCheck(fedd_assemble_advection_ale(dev->ctx, FEDD_ALE_P, 1., -1, 3), "fedd_assemble_advection_ale");
        A->bindSlot(dev, 3);
        A->markAdditionalConvection(++dev->aleSerial);
        if (!callFillComplete) A->resumeFill();
    }
    // FE::assemblyDivAndDivT (FE_def.hpp:1932-2057): velocity = FEType1 on the first domain, pressure = P1 on the vertices,
    // which are the first nodes of a P2-of-P1 velocity domain.  B and B^T land in slots 1 and 2 of the velocity domain's
    // device context (the system slot is scratch for the node pattern), unscaled.
    void assemblyDivAndDivT(int dim, std::string FEType1, std::string FEType2, int degree, MatrixPtr_Type& Bmat, MatrixPtr_Type& BTmat,
                            Teuchos::RCP<const Map<LO, GO, NO>> map1, Teuchos::RCP<const Map<LO, GO, NO>> map2, bool callFillComplete = true) {
        (void)degree; (void)map1; (void)callFillComplete;
        TEUCHOS_TEST_FOR_EXCEPTION(FEType2 != "P1", std::logic_error, "assemblyDivAndDivT: the pressure space of this build is P1");
        const UN loc1 = checkFE(dim, FEType1);
        auto dom = domainVec_.at(loc1);
        const int64_t n_p = (int64_t)map2->getNodeNumElements();
        if (dom->isStructuredP2()) {
            // two structured domains of the same N, M: pressure node k must sit on velocity node k (vertices first), bit for bit, and
            // the element lists must walk in step (the vertices of velocity element T are the nodes of pressure element T)
            auto domP = domainVec_.at(checkFE(dim, FEType2));
            const std::vector<double>& xv = dom->xyzRepeated();
            const std::vector<double>& xp = domP->xyzRepeated();
            bool same = n_p == dom->numberOfP1Nodes() && (int64_t)xp.size() == n_p * dim && domP->getNumElements() == dom->getNumElements() &&
                        std::memcmp(xv.data(), xp.data(), xp.size() * sizeof(double)) == 0;
            const int nenV = dom->nodesPerElement(), nenP = domP->nodesPerElement();
            for (LO T = 0; same && T < dom->getNumElements(); ++T)
                for (int v = 0; v <= dim; ++v) same = same && dom->connectivity()[(size_t)T * nenV + v] == domP->connectivity()[(size_t)T * nenP + v];
            TEUCHOS_TEST_FOR_EXCEPTION(!same, std::logic_error, "assemblyDivAndDivT: the structured P2 velocity domain and the P1 pressure domain "
                                       "do not match (same N and M are needed: pressure node k must be velocity node k, coordinates bit for bit)");
        }
        feddCheck(fedd_set_option(dom->device()->ctx, "asm_zero_eps", setZeros_ ? myeps_ : 0.), "fedd_set_option");   // (FE_def.hpp:2002-2004, 2032-2034)
        feddCheck(fedd_assemble_div(dom->device()->ctx, n_p, 1, 2), "fedd_assemble_div");
        dom->device()->generation++;
        Bmat->bindSlot(dom->device(), 1);
        BTmat->bindSlot(dom->device(), 2);
    }
    // FE::assemblyRHS (FE_def.hpp:4694-4766): f evaluated once (constant); a lives on the REPEATED
    // map in the reference and is then export-added; here the owned entries are produced directly,
    // `a` must live on the unique (vec-field) map.
    void assemblyRHS(int dim, std::string FEType, MultiVectorPtr_Type a, std::string fieldType, RhsFunc_Type func, std::vector<SC>& funcParameter) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType == "P0", std::logic_error, "Not implemented for P0");
        TEUCHOS_TEST_FOR_EXCEPTION(a.is_null(), std::runtime_error, "MultiVector in assemblyConstRHS is null.");
        TEUCHOS_TEST_FOR_EXCEPTION(a->getNumVectors() > 1, std::logic_error, "Implement for numberMV > 1 .");
        const UN loc = checkFE(dim, FEType);
        const int dofs = fieldType == "Scalar" ? 1 : (fieldType == "Vector" ? dim : 0);
        TEUCHOS_TEST_FOR_EXCEPTION(dofs == 0, std::logic_error, "Invalid field type.");
        const int degFunc = (int)(funcParameter[funcParameter.size() - 1] + 1.e-14);
        double x = 0., f[3] = {0, 0, 0};
        func(&x, f, funcParameter.data());            // "for now just const!" (FE_def.hpp:4731-4736)
        fedd_ctx* ctx = domainVec_[loc]->device()->ctx;
        int64_t nr = 0, nc = 0, nnz = 0;
        if (fedd_csr_sizes(ctx, &nr, &nc, &nnz) != 0 || nr != (int64_t)a->getLocalLength()) {
            int64_t dummy;                             // rhs before any matrix: build the matching pattern
            feddCheck(fedd_pattern_build(ctx, dofs, dofs == 1 ? FEDD_BLOCK_SCALAR : FEDD_BLOCK_DIAG, &dummy), "fedd_pattern_build");
            domainVec_[loc]->device()->generation++;
        }
        feddCheck(fedd_assemble_rhs(ctx, dofs, f, degFunc), "fedd_assemble_rhs");
        feddCheck(fedd_rhs_get(ctx, a->raw().data()), "fedd_rhs_get");
    }
    // FE::assemblySurfaceIntegral (FE_def.hpp:4511-4599): int_Gamma func . phi_i over every surface element of the domain.  The
    // callback is evaluated once per surface element, at its first quadrature point, with the element's flag in
    // funcParameter[size - 2]; the last entry is the degree of the function, and only constant functions are taken.  `a` lives
    // on the unique (vec-field) map, as in assemblyRHS above.
    void assemblySurfaceIntegral(int dim, std::string FEType, MultiVectorPtr_Type f, std::string fieldType, RhsFunc_Type func, std::vector<SC>& funcParameter) {
        TEUCHOS_TEST_FOR_EXCEPTION(funcParameter.size() < 2, std::logic_error, "assemblySurfaceIntegral: the parameters need a slot for the surface flag before the degree.");
        TEUCHOS_TEST_FOR_EXCEPTION(funcParameter[funcParameter.size() - 1] > 0., std::logic_error, "We only support constant functions for now.");
        const int degFunc = (int)(funcParameter[funcParameter.size() - 1] + 1.e-14);
        SC* params = funcParameter.data();
        surfaceIntegral(dim, FEType, f, fieldType, degFunc, [&](double* x, double* res, int flag) {
            params[funcParameter.size() - 2] = flag;
            func(x, res, params);
            return true;
        });
    }
    // FE::assemblySurfaceIntegralFlag (FE_def.hpp:4601-4691): the same over the surface elements that carry the flag
    // funcParameter[2]; funcParameter = {order, time, flag}
    void assemblySurfaceIntegralFlag(int dim, std::string FEType, MultiVectorPtr_Type f, std::string fieldType, BC_func_Type func, std::vector<SC>& funcParameter) {
        TEUCHOS_TEST_FOR_EXCEPTION(funcParameter.size() < 3, std::logic_error, "assemblySurfaceIntegralFlag: parameters are {order, time, flag}.");
        TEUCHOS_TEST_FOR_EXCEPTION(funcParameter[0] != 0, std::logic_error, "We only support constant functions for now.");
        SC* params = &funcParameter[1];
        surfaceIntegral(dim, FEType, f, fieldType, 0, [&](double* x, double* res, int flag) {
            if (params[1] != flag) return false;
            func(x, res, params[0], params);
            return true;
        });
    }
private:
    // eval(x, res, flag): the load of a surface element at the point x, false = the element is left out
    template <class Eval>
    void surfaceIntegral(int dim, const std::string& FEType, MultiVectorPtr_Type f, const std::string& fieldType, int degFunc, Eval eval) {
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P1" && FEType != "P2", std::logic_error, "Surface integrals are built for P1 and P2.");
        TEUCHOS_TEST_FOR_EXCEPTION(f.is_null(), std::runtime_error, "MultiVector in assemblySurfaceIntegral is null.");
        const UN loc = checkFE(dim, FEType);
        auto dom = domainVec_[loc];
        const int dofs = fieldType == "Scalar" ? 1 : (fieldType == "Vector" ? dim : 0);
        TEUCHOS_TEST_FOR_EXCEPTION(dofs == 0, std::logic_error, "Invalid field type.");
        TEUCHOS_TEST_FOR_EXCEPTION((size_t)f->getLocalLength() != (size_t)dom->getMapUnique()->getNodeNumElements() * dofs, std::logic_error,
                                   "assemblySurfaceIntegral: the vector does not live on the unique map of a '" << fieldType << "' field.");
        const int nsn = dom->nodesPerSurfaceElement();
        const auto& surf = dom->surfaceElements();
        const auto& sflag = dom->surfaceFlags();
        const auto& xyz = dom->xyzRepeated();
        // first quadrature point of the surface rule, degree determineDegree(dim-1, FEType, Std) + degFunc (:4530-4537)
        int nq = 0;
        const int deg = (FEType == "P2" ? 2 : 1) + degFunc;
        feddCheck(fedd_fe_quadrature(dim - 1, deg, &nq, nullptr, nullptr), "fedd_fe_quadrature");
        std::vector<double> q((size_t)nq * (dim - 1)), w((size_t)nq);
        feddCheck(fedd_fe_quadrature(dim - 1, deg, &nq, q.data(), w.data()), "fedd_fe_quadrature");
        std::vector<double> g(sflag.size() * dofs, 0.);
        std::vector<double> valueFunc(dim, 0.), x(dim, 0.);
        for (size_t s = 0; s < sflag.size(); ++s) {
            // x = b + B q.  (The reference adds b once per column of B, :4570-4573 -- x = 2 b + B q in 3D --, which is wrong there
            // and immaterial for the constant functions it admits.)
            const int32_t n0 = surf[s * nsn];
            for (int k = 0; k < dim; ++k) {
                x[k] = xyz[(size_t)n0 * dim + k];
                for (int l = 0; l < dim - 1; ++l) x[k] += (xyz[(size_t)surf[s * nsn + l + 1] * dim + k] - xyz[(size_t)n0 * dim + k]) * q[l];
            }
            if (!eval(x.data(), valueFunc.data(), sflag[s])) continue;
            for (int d = 0; d < dofs; ++d) g[s * dofs + d] = valueFunc[d];
        }
        fedd_ctx* ctx = dom->device()->ctx;
        int64_t nr = 0, nc = 0, nnz = 0;
        if (fedd_csr_sizes(ctx, &nr, &nc, &nnz) != 0 || nr != (int64_t)f->getLocalLength()) {
            int64_t dummy;                             // load vector before any matrix: build the matching pattern
            feddCheck(fedd_pattern_build(ctx, dofs, dofs == 1 ? FEDD_BLOCK_SCALAR : FEDD_BLOCK_DIAG, &dummy), "fedd_pattern_build");
            dom->device()->generation++;
        }
        feddCheck(fedd_assemble_surface_values(ctx, dofs, g.data(), degFunc, 0), "fedd_assemble_surface_values");
        feddCheck(fedd_rhs_get(ctx, f->raw().data()), "fedd_rhs_get");
    }
    void assembleInto(UN loc, int dofs, int mode, int form, const double* params, MatrixPtr_Type& A, bool callFillComplete) {
        TEUCHOS_TEST_FOR_EXCEPTION(A.is_null(), std::runtime_error, "Matrix is null.");
        auto dom = domainVec_.at(loc);
        TEUCHOS_TEST_FOR_EXCEPTION((size_t)A->getMap()->getNodeNumElements() != (size_t)dom->getMapUnique()->getNodeNumElements() * dofs,
                                   std::logic_error, "Matrix row map does not match the unique map of the domain.");
        fedd_ctx* ctx = dom->device()->ctx;
        int64_t nnz;
        feddCheck(fedd_pattern_build(ctx, dofs, mode, &nnz), "fedd_pattern_build");
        feddCheck(fedd_assemble(ctx, form, params), "fedd_assemble");
        dom->device()->generation++;
        A->bind(dom->device(), dofs);
        if (!callFillComplete) A->resumeFill();
    }
    std::vector<DomainConstPtr_Type> domainVec_;
    bool setZeros_ = false;
    double myeps_ = 0.;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class BCBuilder {
public:
    typedef Domain<SC, LO, GO, NO> Domain_Type;
    typedef Teuchos::RCP<Domain_Type> DomainPtr_Type;
    typedef Teuchos::RCP<const Domain_Type> DomainConstPtr_Type;
    typedef BlockMatrix<SC, LO, GO, NO> BlockMatrix_Type;
    typedef Teuchos::RCP<BlockMatrix_Type> BlockMatrixPtr_Type;
    typedef BlockMultiVector<SC, LO, GO, NO> BlockMultiVector_Type;
    typedef Teuchos::RCP<BlockMultiVector_Type> BlockMultiVectorPtr_Type;

    BCBuilder() {}
    void addBC(BC_func_Type funcBC, int flag, int block, const DomainPtr_Type& domain, std::string type, int dofs) {
        vec_dbl_Type dummy(1, 0.);
        addBC(funcBC, flag, block, domain, type, dofs, dummy);
    }
    void addBC(BC_func_Type funcBC, int flag, int block, const DomainPtr_Type& domain, std::string type, int dofs, vec_dbl_Type& parameter_vec) {
        vecBC_func_.push_back(funcBC); vecFlag_.push_back(flag); vecBlockID_.push_back(block); vecDomain_.push_back(domain);
        vecBCType_.push_back(type); vecDofs_.push_back(dofs); vecBC_Parameters_.push_back(parameter_vec);
    }
    bool findFlag(LO flag, int block, int& loc) const {   // BCBuilder_def.hpp findFlag
        for (size_t i = 0; i < vecFlag_.size(); ++i)
            if (vecFlag_[i] == flag && vecBlockID_[i] == block) { loc = (int)i; return true; }
        return false;
    }
    bool blockHasDirichletBC(int block) const { int l; return blockHasDirichletBC(block, l); }
    bool blockHasDirichletBC(int block, int& loc) const {
        for (size_t i = 0; i < vecBlockID_.size(); ++i)
            if (vecBlockID_[i] == block && vecBCType_[i].compare(0, 9, "Dirichlet") == 0) { loc = (int)i; return true; }
        return false;
    }
    // (set() adds the "Neumann" entries, and so does setRHS(): call one of them on a right-hand side, not both, or the
    // Neumann vector is added twice)
    // BCBuilder::set = setSystem + setRHS (BCBuilder_def.hpp:84-90).  The device call does both for
    // the diagonal block; the host evaluates the user function at every flagged unique node.
    void set(const BlockMatrixPtr_Type& blockMatrix, const BlockMultiVectorPtr_Type& blockMV, double t = 0.) const {
        TEUCHOS_TEST_FOR_EXCEPTION(blockMV->getNumVectors() > 1, std::runtime_error, "BCBuilder::setRHS() only for getNumVectors == 1.");
        for (UN block = 0; block < blockMatrix->size(); ++block) {
            addNeumann(blockMV, (int)block, t);     // before the Dirichlet treatment, which overwrites
            int loc0;
            if (!blockHasDirichletBC((int)block, loc0)) continue;
            if (blockMatrix->size() > 1) {
                // merged block system on the device: unit row on the merged row, i.e. setLocalRowOne on the diagonal block and
                // setLocalRowZero on the off-diagonal blocks (BCBuilder_def.hpp:653-707), rhs <- boundary value
                setMerged(blockMatrix, blockMV, (int)block, t);
                continue;
            }
            auto A = blockMatrix->getBlock(block, block);
            TEUCHOS_TEST_FOR_EXCEPTION(!A->isResident(), std::runtime_error, "BCBuilder: the matrix block is not resident on the device");
            auto dom = vecDomain_.at(loc0);
            const int dofs = vecDofs_.at(loc0), dim = (int)dom->getDimension();
            vec_int_ptr_Type flags = dom->getBCFlagUnique();
            vec2D_dbl_ptr_Type pts = dom->getPointsUnique();
            std::vector<int32_t> nodes, mask;
            std::vector<double> values;
            vec_dbl_Type result(dofs, 0.), point(dim, 0.);
            // owned nodes, then (several ranks) the row ghosts: their rows exist on this rank and get the same treatment
            const auto& rgRep = dom->rowGhostRepeatedIds();
            const auto& rgFlag = dom->rowGhostFlags();
            const auto& xyzRep = dom->xyzRepeated();
            const size_t nOwned = flags->size();
            for (size_t i = 0; i < nOwned + rgRep.size(); ++i) {
                int loc;
                const int flag = i < nOwned ? (*flags)[i] : rgFlag[i - nOwned];
                if (!findFlag(flag, (int)block, loc)) continue;
                const std::string& ty = vecBCType_[loc];
                if (ty.compare(0, 9, "Dirichlet") != 0) continue;
                for (int d = 0; d < dim; ++d) point[d] = i < nOwned ? (*pts)[i][d] : xyzRep[(size_t)rgRep[i - nOwned] * dim + d];
                for (int d = 0; d < dofs; ++d) result[d] = d < dim ? point[d] : 0.;   // :136-138
                vecBC_func_[loc](point.data(), result.data(), t, vecBC_Parameters_[loc].data());
                nodes.push_back((int32_t)i);
                for (int d = 0; d < dofs; ++d) {
                    const bool on = ty == "Dirichlet" || (ty == "Dirichlet_X" && d == 0) || (ty == "Dirichlet_Y" && d == 1) ||
                                    (ty == "Dirichlet_Z" && d == 2) || (ty == "Dirichlet_X_Y" && d != 2) ||
                                    (ty == "Dirichlet_X_Z" && d != 1) || (ty == "Dirichlet_Y_Z" && d != 0);
                    mask.push_back(on ? 1 : 0);
                    values.push_back(result[d]);
                }
            }
            fedd_ctx* ctx = A->device()->ctx;
            // push the current rhs, apply rows + rhs on the device, pull the rhs back
            feddCheck(fedd_rhs_set(ctx, blockMV->getBlockNonConst(block)->raw().data()), "fedd_rhs_set");
            feddCheck(fedd_dirichlet_nodes(ctx, (int64_t)nodes.size(), nodes.data(), mask.data(), values.data()), "fedd_dirichlet_nodes");
            feddCheck(fedd_rhs_get(ctx, blockMV->getBlockNonConst(block)->raw().data()), "fedd_rhs_get");
            A->invalidateHost();
        }
    }
    // the Dirichlet rows of `block` in the numbering of the merged system (the blocks one after the other) and their values
    void mergedDirichletRows(const BlockMultiVectorPtr_Type& blockMV, int block, double t, std::vector<int32_t>& rows,
                             std::vector<double>& values) const {
        int64_t rowOffset = 0;
        for (int b = 0; b < block; ++b) rowOffset += (int64_t)blockMV->getBlock(b)->getLocalLength();
        for (size_t k = 0; k < vecFlag_.size(); ++k) {
            if (vecBlockID_[k] != block || vecBCType_[k].compare(0, 9, "Dirichlet") != 0) continue;
            auto dom = vecDomain_[k];
            const int dofs = vecDofs_[k], dim = (int)dom->getDimension();
            vec_int_ptr_Type flags = dom->getBCFlagUnique();
            vec2D_dbl_ptr_Type pts = dom->getPointsUnique();
            const std::string& ty = vecBCType_[k];
            vec_dbl_Type result(dofs, 0.), point(dim, 0.);
            for (size_t i = 0; i < flags->size(); ++i) {
                if ((*flags)[i] != vecFlag_[k]) continue;
                for (int d = 0; d < dim; ++d) point[d] = (*pts)[i][d];
                for (int d = 0; d < dofs; ++d) result[d] = d < dim ? (*pts)[i][d] : 0.;
                vecBC_func_[k](point.data(), result.data(), t, vecBC_Parameters_[k].data());
                for (int d = 0; d < dofs; ++d) {
                    const bool on = ty == "Dirichlet" || (ty == "Dirichlet_X" && d == 0) || (ty == "Dirichlet_Y" && d == 1) ||
                                    (ty == "Dirichlet_Z" && d == 2) || (ty == "Dirichlet_X_Y" && d != 2) ||
                                    (ty == "Dirichlet_X_Z" && d != 1) || (ty == "Dirichlet_Y_Z" && d != 0);
                    if (!on) continue;
                    rows.push_back((int32_t)(rowOffset + (int64_t)i * dofs + d));
                    values.push_back(result[d]);
                }
            }
        }
    }
    // BCBuilder::setSystem alone on a merged block system (BCBuilder_def.hpp:589-707): unit rows, no right-hand side
    void setSystem(const BlockMatrixPtr_Type& blockMatrix, const BlockMultiVectorPtr_Type& layout) const {
        auto dev = blockMatrix->mergedDevice();
        if (blockMatrix->size() == 1 && dev.is_null()) {
            // one block (nonlinear elasticity): the unit rows of set() on the resident matrix; the right-hand side stays as it is
            BlockMultiVectorPtr_Type scratch(new BlockMultiVector_Type(1));
            scratch->addBlock(Teuchos::rcp(new MultiVector<SC, LO, GO, NO>(layout->getBlock(0)->getMap(), 1)), 0);
            set(blockMatrix, scratch, 0.);
            return;
        }
        TEUCHOS_TEST_FOR_EXCEPTION(dev.is_null(), std::runtime_error, "BCBuilder: the block system has not been merged on the device");
        std::vector<int32_t> rows;
        std::vector<double> values;
        for (UN b = 0; b < blockMatrix->size(); ++b) mergedDirichletRows(layout, (int)b, 0., rows, values);
        std::fill(values.begin(), values.end(), 0.);
        feddCheck(fedd_dirichlet_rows(dev->ctx, (int64_t)rows.size(), rows.data(), values.data()), "fedd_dirichlet_rows");
    }
    // the Dirichlet rows of one block in the merged numbering (block 0: the block's own numbering), values at time 0
    void dirichletRowsOfBlock(const BlockMultiVectorPtr_Type& layout, int block, std::vector<int32_t>& rows, std::vector<double>& values) const {
        mergedDirichletRows(layout, block, 0., rows, values);
    }
    // the Dirichlet conditions of `block` as fedd_newton_residual takes them: per flag a component mask and one value per
    // component.  A boundary function that varies over the nodes of a flag does not fit that table: an error that says so.
    void dirichletFlagTable(int block, double t, std::vector<int32_t>& flags, std::vector<int32_t>& mask, std::vector<double>& values) const {
        for (size_t k = 0; k < vecFlag_.size(); ++k) {
            if (vecBlockID_[k] != block || vecBCType_[k].compare(0, 9, "Dirichlet") != 0) continue;
            auto dom = vecDomain_[k];
            const int dofs = vecDofs_[k], dim = (int)dom->getDimension();
            vec_int_ptr_Type nodeFlags = dom->getBCFlagUnique();
            vec2D_dbl_ptr_Type pts = dom->getPointsUnique();
            const std::string& ty = vecBCType_[k];
            vec_dbl_Type result(dofs, 0.), point(dim, 0.), first;
            for (size_t i = 0; i < nodeFlags->size(); ++i) {
                if ((*nodeFlags)[i] != vecFlag_[k]) continue;
                for (int d = 0; d < dim; ++d) point[d] = (*pts)[i][d];
                for (int d = 0; d < dofs; ++d) result[d] = d < dim ? (*pts)[i][d] : 0.;
                vecBC_func_[k](point.data(), result.data(), t, vecBC_Parameters_[k].data());
                if (first.empty()) first = result;
                for (int d = 0; d < dofs; ++d) {
                    const bool on = ty == "Dirichlet" || (ty == "Dirichlet_X" && d == 0) || (ty == "Dirichlet_Y" && d == 1) ||
                                    (ty == "Dirichlet_Z" && d == 2) || (ty == "Dirichlet_X_Y" && d != 2) ||
                                    (ty == "Dirichlet_X_Z" && d != 1) || (ty == "Dirichlet_Y_Z" && d != 0);
                    TEUCHOS_TEST_FOR_EXCEPTION(on && result[d] != first[d], std::logic_error,
                                               "Dirichlet values that vary over the nodes of flag " + std::to_string(vecFlag_[k]) +
                                               " are not built for the device-resident Newton residual (one value per flag and component is)");
                }
            }
            if (first.empty()) continue;
            flags.push_back(vecFlag_[k]);
            for (int d = 0; d < dofs; ++d) {
                const bool on = ty == "Dirichlet" || (ty == "Dirichlet_X" && d == 0) || (ty == "Dirichlet_Y" && d == 1) ||
                                (ty == "Dirichlet_Z" && d == 2) || (ty == "Dirichlet_X_Y" && d != 2) ||
                                (ty == "Dirichlet_X_Z" && d != 1) || (ty == "Dirichlet_Y_Z" && d != 0);
                mask.push_back(on ? 1 : 0);
                values.push_back(first[d]);
            }
        }
    }
    // BCBuilder::setRHS (:93-170), setVectorMinusBC and setBCMinusVector (the boundary rows of a nonlinear residual):
    // which = 0: v <- g, 1: v <- x - g, 2: v <- g - x on the Dirichlet rows
    void setRows(const BlockMultiVectorPtr_Type& v, const BlockMultiVectorPtr_Type& x, double t, int which) const {
        std::vector<int32_t> rows;
        std::vector<double> values;
        for (UN b = 0; b < v->size(); ++b) mergedDirichletRows(v, (int)b, t, rows, values);
        std::vector<int64_t> start(v->size() + 1, 0);
        for (UN b = 0; b < v->size(); ++b) start[b + 1] = start[b] + (int64_t)v->getBlock(b)->getLocalLength();
        for (size_t k = 0; k < rows.size(); ++k) {
            UN b = 0;
            while (rows[k] >= start[b + 1]) ++b;
            const size_t i = (size_t)(rows[k] - start[b]);
            double& dst = v->getBlockNonConst(b)->raw()[i];
            const double xi = which == 0 ? 0. : x->getBlock(b)->raw()[i];
            dst = which == 0 ? values[k] : (which == 1 ? xi - values[k] : values[k] - xi);
        }
    }
    // (adds the "Neumann" entries like set(): not to be called on a right-hand side that set() has already treated)
    void setRHS(const BlockMultiVectorPtr_Type& rhs, double t = 0.) const {
        for (UN b = 0; b < rhs->size(); ++b) addNeumann(rhs, (int)b, t);
        setRows(rhs, rhs, t, 0);
    }
    void setVectorMinusBC(const BlockMultiVectorPtr_Type& v, const BlockMultiVectorPtr_Type& x, double t = 0.) const { setRows(v, x, t, 1); }
    void setBCMinusVector(const BlockMultiVectorPtr_Type& v, const BlockMultiVectorPtr_Type& x, double t = 0.) const { setRows(v, x, t, 2); }
private:
    // the "Neumann" entries of a block (BCBuilder::setRHS, BCBuilder_def.hpp:172-199): rhs += int_Gamma_flag g . phi_i, with
    // funcParameter = {order 0, time, flag}.  The domain's device context computes it; a matrix of the same dofs stays untouched.
    void addNeumann(const BlockMultiVectorPtr_Type& blockMV, int block, double t) const {
        for (size_t i = 0; i < vecBCType_.size(); ++i) {
            if (vecBCType_[i] != "Neumann" || vecBlockID_[i] != block) continue;
            DomainPtr_Type domain = vecDomain_[i];
            FE<SC, LO, GO, NO> feFactory;
            feFactory.addFE(domain);
            std::vector<SC> funcParameter(3, 0.);
            funcParameter[1] = t;
            funcParameter[2] = vecFlag_[i];
            const int dim = (int)domain->getDimension(), dofs = vecDofs_[i];
            auto aUnique = Teuchos::rcp(new MultiVector<SC, LO, GO, NO>(dofs > 1 ? domain->getMapVecFieldUnique() : domain->getMapUnique()));
            feFactory.assemblySurfaceIntegralFlag(dim, domain->getFEType(), aUnique, dofs > 1 ? "Vector" : "Scalar", vecBC_func_[i], funcParameter);
            blockMV->getBlockNonConst(block)->update(1., *aUnique, 1.);
        }
    }
    void setMerged(const BlockMatrixPtr_Type& blockMatrix, const BlockMultiVectorPtr_Type& blockMV, int block, double t) const {
        auto dev = blockMatrix->mergedDevice();
        TEUCHOS_TEST_FOR_EXCEPTION(dev.is_null(), std::runtime_error, "BCBuilder: the block system has not been merged on the device");
        std::vector<int32_t> rows;
        std::vector<double> values;
        mergedDirichletRows(blockMV, block, t, rows, values);
        // the merged rhs = the blocks' right-hand sides one after the other
        std::vector<double> rhs;
        for (UN b = 0; b < blockMV->size(); ++b) rhs.insert(rhs.end(), blockMV->getBlock(b)->raw().begin(), blockMV->getBlock(b)->raw().end());
        feddCheck(fedd_rhs_set(dev->ctx, rhs.data()), "fedd_rhs_set");
        feddCheck(fedd_dirichlet_rows(dev->ctx, (int64_t)rows.size(), rows.data(), values.data()), "fedd_dirichlet_rows");
        feddCheck(fedd_rhs_get(dev->ctx, rhs.data()), "fedd_rhs_get");
        size_t off = 0;
        for (UN b = 0; b < blockMV->size(); ++b) {
            auto& dst = blockMV->getBlockNonConst(b)->raw();
            std::copy(rhs.begin() + off, rhs.begin() + off + dst.size(), dst.begin());
            off += dst.size();
        }
    }
    std::vector<BC_func_Type> vecBC_func_;
    std::vector<int> vecFlag_, vecBlockID_, vecDofs_;
    std::vector<DomainPtr_Type> vecDomain_;
    std::vector<std::string> vecBCType_;
    std::vector<vec_dbl_Type> vecBC_Parameters_;
};

template <class SC, class LO, class GO, class NO>
class Problem;

// PreconditionerOperator (feddlib/problems/Solver/PreconditionerOperator_decl.hpp:24-125): the reference's base class for a
// preconditioner that the user hands to the iterative solver through Problem::setPreconditionerThyraFromLinOp
// (Problem_def.hpp:397-399, Preconditioner_def.hpp:96-102) -- there a Thyra::LinearOpBase with a pure applyImpl, here the
// same contract on the facade's MultiVector:  Y = alpha * M^-1 X + beta * Y  on the entries of the unique map.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class PreconditionerOperator {
public:
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    virtual ~PreconditionerOperator() {}
    void apply(const MultiVector_Type& X, MultiVector_Type& Y, SC alpha = 1., SC beta = 0.) const { applyImpl(X, Y, alpha, beta); }
    virtual std::string description() const { return "FEDD::PreconditionerOperator"; }
protected:
    virtual void applyImpl(const MultiVector_Type& X, MultiVector_Type& Y, const SC alpha, const SC beta) const = 0;
};

// the library's Schwarz preconditioner behind that interface.  Every application crosses the host
// boundary (fedd_schwarz_apply takes and returns host vectors); the resident path is LinearSolver's default.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class DeviceSchwarzOperator : public PreconditionerOperator<SC, LO, GO, NO> {
public:
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    // the matrix resident in `dev` must be final (assembled, boundary conditions set); parameters as in parametersPrec.xml
    DeviceSchwarzOperator(const DeviceContextPtr& dev, int overlap = 1, const std::string& combine = "Restricted", bool twoLevel = false,
                          int coarseKind = FEDD_COARSE_GDSW)
        : dev_(dev) {
        const int cmb = combine == "Averaging" ? FEDD_COMBINE_AVERAGING : (combine == "Full" ? FEDD_COMBINE_FULL : FEDD_COMBINE_RESTRICTED);
        feddCheck(fedd_schwarz_setup(dev_->ctx, overlap, cmb, twoLevel ? 1 : 0, twoLevel ? coarseKind : 0), "fedd_schwarz_setup");
    }
    std::string description() const override { return "FEDD::DeviceSchwarzOperator (overlapping Schwarz on the GPU)"; }
protected:
    void applyImpl(const MultiVector_Type& X, MultiVector_Type& Y, const SC alpha, const SC beta) const override {
        z_.resize(X.raw().size());
        feddCheck(fedd_schwarz_apply(dev_->ctx, X.raw().data(), z_.data()), "fedd_schwarz_apply");
        auto& y = Y.raw();
        for (size_t i = 0; i < y.size(); ++i) y[i] = alpha * z_[i] + (beta == 0. ? 0. : beta * y[i]);
    }
private:
    DeviceContextPtr dev_;
    mutable std::vector<SC> z_;
};

// LinearSolver::solve -> solveMonolithic (LinearSolver_def.hpp:23-135): GMRES + one-level Schwarz on
// the device, configured from the same ParameterList entries the reference hands to Stratimikos.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class LinearSolver {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef BlockMultiVector<SC, LO, GO, NO> BlockMultiVector_Type;
    typedef Teuchos::RCP<BlockMultiVector_Type> BlockMultiVectorPtr_Type;
    int solve(Problem_Type* problem, BlockMultiVectorPtr_Type rhs, std::string type = "Monolithic");
    // the FROSch keys of one "ThyraPreconditioner" list -> fedd_schwarz_set_* + fedd_schwarz_setup on one context (the merged
    // system, or a block of it)
    static void setupSchwarz(fedd_ctx* ctx, Teuchos::ParameterList& thyraPrec, Teuchos::ParameterList& pl, bool blocks, bool verbose);
    static int combineMode(Teuchos::ParameterList& frosch);
    // "Diagonal" / "Triangular": children, import, pressure mass matrix, setups, attach (PrecBlock2x2)
    static void setupBlockPreconditioner(Problem_Type* problem, fedd_ctx* ctx, const std::string& type);
    double lastRelativeResidual = 0.;
private:
    typedef MultiVector<SC, LO, GO, NO> MV;
    static double dot(const MV& a, const MV& b) {
        double s = 0.;
        const auto& x = a.raw();
        const auto& y = b.raw();
        for (size_t i = 0; i < x.size(); ++i) s += x[i] * y[i];
        if (!a.getMap()->getComm().is_null()) a.getMap()->getComm()->sumAll(&s, 1);
        return s;
    }
    static int hostGmres(Matrix<SC, LO, GO, NO>& A, const PreconditionerOperator<SC, LO, GO, NO>& M, const MV& b, MV& x, double tol,
                         int maxIt, int m, double& rel) {
        auto map = b.getMap();
        const double bnorm = b.norm2();
        x.putScalar(0.);
        rel = 0.;
        if (bnorm == 0.) return 0;
        MV r(map), z(map), w(map);
        r.update(1., b, 0.);
        double beta = bnorm;
        int its = 0;
        while (its < maxIt) {
            std::vector<MV> V;
            V.reserve((size_t)m + 1);
            V.emplace_back(map);
            V[0].update(1. / beta, r, 0.);
            std::vector<std::vector<double>> H((size_t)m, std::vector<double>((size_t)m + 1, 0.));
            std::vector<double> cs((size_t)m, 0.), sn((size_t)m, 0.), g((size_t)m + 1, 0.);
            g[0] = beta;
            int k = 0;
            for (; k < m && its < maxIt; ++k) {
                M.apply(V[k], z);
                A.apply(z, w);
                for (int pass = 0; pass < 2; ++pass) {       // classical Gram-Schmidt, twice
                    std::vector<double> h((size_t)k + 1);
                    for (int i = 0; i <= k; ++i) h[i] = dot(V[i], w);
                    for (int i = 0; i <= k; ++i) {
                        w.update(-h[i], V[i], 1.);
                        H[k][i] += h[i];
                    }
                }
                const double hn = w.norm2();
                H[k][k + 1] = hn;
                for (int i = 0; i < k; ++i) {
                    const double t = cs[i] * H[k][i] + sn[i] * H[k][i + 1];
                    H[k][i + 1] = -sn[i] * H[k][i] + cs[i] * H[k][i + 1];
                    H[k][i] = t;
                }
                const double d = std::hypot(H[k][k], H[k][k + 1]);
                cs[k] = H[k][k] / d;
                sn[k] = H[k][k + 1] / d;
                H[k][k] = d;
                H[k][k + 1] = 0.;
                g[k + 1] = -sn[k] * g[k];
                g[k] = cs[k] * g[k];
                ++its;
                rel = std::fabs(g[k + 1]) / bnorm;
                if (rel <= tol || hn == 0.) { ++k; break; }
                V.emplace_back(map);
                V[k + 1].update(1. / hn, w, 0.);
            }
            std::vector<double> y((size_t)k, 0.);
            for (int i = k - 1; i >= 0; --i) {
                double sum = g[i];
                for (int j = i + 1; j < k; ++j) sum -= H[j][i] * y[j];
                y[i] = sum / H[i][i];
            }
            w.putScalar(0.);
            for (int i = 0; i < k; ++i) w.update(y[i], V[i], 1.);
            M.apply(w, z);
            x.update(1., z, 1.);
            if (rel <= tol) break;
            A.apply(x, w);
            r.update(1., b, 0.);
            r.update(-1., w, 1.);
            beta = r.norm2();
            rel = beta / bnorm;
            if (rel <= tol) break;
        }
        return its;
    }
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Problem {
public:
    typedef Domain<SC, LO, GO, NO> Domain_Type;
    typedef Teuchos::RCP<const Domain_Type> DomainConstPtr_Type;
    typedef std::vector<DomainConstPtr_Type> DomainConstPtr_vec_Type;
    typedef Matrix<SC, LO, GO, NO> Matrix_Type;
    typedef Teuchos::RCP<Matrix_Type> MatrixPtr_Type;
    typedef BlockMatrix<SC, LO, GO, NO> BlockMatrix_Type;
    typedef Teuchos::RCP<BlockMatrix_Type> BlockMatrixPtr_Type;
    typedef MultiVector<SC, LO, GO, NO> MultiVector_Type;
    typedef Teuchos::RCP<MultiVector_Type> MultiVectorPtr_Type;
    typedef BlockMultiVector<SC, LO, GO, NO> BlockMultiVector_Type;
    typedef Teuchos::RCP<BlockMultiVector_Type> BlockMultiVectorPtr_Type;
    typedef BCBuilder<SC, LO, GO, NO> BC_Type;
    typedef Teuchos::RCP<const BC_Type> BCConstPtr_Type;
    typedef FE<SC, LO, GO, NO> FEFac_Type;
    typedef Teuchos::RCP<FEFac_Type> FEFacPtr_Type;
    typedef Teuchos::Comm<int> Comm_Type;
    typedef Teuchos::RCP<const Comm_Type> CommConstPtr_Type;

    Problem(ParameterListPtr_Type& parameterList, CommConstPtr_Type comm)
        : dim_(-1), comm_(comm), verbose_(comm->getRank() == 0), parameterList_(parameterList), feFactory_(new FEFac_Type()) {}
    virtual ~Problem() {}
    virtual void info() = 0;
    void infoProblem() {
        if (verbose_) {
            std::cout << "\t ### Problem Information ###" << std::endl;
            for (size_t i = 0; i < domainPtr_vec_.size(); ++i)
                std::cout << "\t ### Variable " << variableName_vec_[i] << ": dofs/node " << dofsPerNode_vec_[i] << ", FE " << domain_FEType_vec_[i] << std::endl;
        }
    }
    void addVariable(const DomainConstPtr_Type& domain, std::string FEType, std::string name, int dofsPerNode) {
        domainPtr_vec_.push_back(domain); domain_FEType_vec_.push_back(FEType); variableName_vec_.push_back(name);
        dofsPerNode_vec_.push_back(dofsPerNode); feFactory_->addFE(domain);
    }
    void addRhsFunction(RhsFunc_Type func) { rhsFuncVec_.push_back(func); }
    RhsFunc_Type& getRhsFunction(int i) { return rhsFuncVec_.at(i); }
    virtual void assemble(std::string type = "") const = 0;

    void assembleSourceTerm(double time = 0.) const {                 // Problem_def.hpp:170-181
        TEUCHOS_TEST_FOR_EXCEPTION(sourceTerm_.is_null(), std::runtime_error, "Initialize source term before you assemble it - sourceTerm pointer is null");
        sourceTerm_->putScalar(0.);
        std::string sourceType = parameterList_->sublist("Parameter").get("Source Type", "volume");
        if (sourceType == "volume") assembleVolumeTerm(time);
        else if (sourceType == "surface") assembleSurfaceTerm(time);
    }
    void assembleSurfaceTerm(double time) const {                     // Problem_def.hpp:219-254
        for (UN i = 0; i < sourceTerm_->size(); ++i) {
            if (i < rhsFuncVec_.size() && rhsFuncVec_[i]) {
                vec_dbl_Type funcParameter(1, 0.);
                funcParameter[0] = time;
                for (double p : parasSourceFunc_) funcParameter.push_back(p);
                // one more slot: the surface flag of the element goes where the degree was, the degree moves to the end
                funcParameter.push_back(funcParameter[funcParameter.size() - 1]);
                // (always "Vector", as in the reference: a surface source of a scalar variable is rejected by the length check)
                feFactory_->assemblySurfaceIntegral((int)getDomain((int)i)->getDimension(), getDomain((int)i)->getFEType(),
                                                    sourceTerm_->getBlockNonConst(i), "Vector", rhsFuncVec_[i], funcParameter);
            }
        }
    }
    void assembleVolumeTerm(double time) const {                      // Problem_def.hpp:184-216
        for (UN i = 0; i < sourceTerm_->size(); ++i) {
            if (i < rhsFuncVec_.size() && rhsFuncVec_[i]) {
                vec_dbl_Type funcParameter(1, 0.);
                funcParameter[0] = time;
                for (double p : parasSourceFunc_) funcParameter.push_back(p);
                const std::string type = getDofsPerNode((int)i) > 1 ? "Vector" : "Scalar";
                feFactory_->assemblyRHS(dim_, domain_FEType_vec_.at(i), sourceTerm_->getBlockNonConst(i), type, rhsFuncVec_[i], funcParameter);
            }
        }
    }
    bool hasSourceTerm() const { return !sourceTerm_.is_null(); }
    // a right-hand-side function was added (what the reference's hasSourceTerm_ flag records, Problem_def.hpp addRhsFunction)
    bool hasRhsFunction() const {
        for (const auto& f : rhsFuncVec_)
            if (f) return true;
        return false;
    }
    int solve(BlockMultiVectorPtr_Type rhs = Teuchos::null) {         // Problem_def.hpp:257-295
        if (verbose_) std::cout << "-- Solve System ..." << std::endl;
        LinearSolver<SC, LO, GO, NO> linSolver;
        std::string type = parameterList_->sublist("General").get("Preconditioner Method", "Monolithic");
        int its = linSolver.solve(this, rhs, type);
        lastRelativeResidual_ = linSolver.lastRelativeResidual;
        if (verbose_) std::cout << " done. -- " << its << " iterations, relative residual " << lastRelativeResidual_ << std::endl;
        return its;
    }
    // Problem::setPreconditionerThyraFromLinOp (Problem_def.hpp:397-399): a user-supplied preconditioner; the solve then
    // runs the host-side GMRES below (the stand-in for Belos in this build) on Matrix::apply and this operator
    typedef PreconditionerOperator<SC, LO, GO, NO> PrecOp_Type;
    void setPreconditionerThyraFromLinOp(const Teuchos::RCP<PrecOp_Type>& op) { userPrec_ = op; }
    Teuchos::RCP<PrecOp_Type> getUserPreconditioner() const { return userPrec_; }
    void addBoundaries(const BCConstPtr_Type& bcFactory) { bcFactory_ = bcFactory; }
    void setBoundaries(double time = .0) const {                      // Problem_def.hpp:298-304
        TEUCHOS_TEST_FOR_EXCEPTION(bcFactory_.is_null(), std::runtime_error, "No boundary conditions added.");
        bcFactory_->set(system_, rhs_, time);
    }
    void initializeProblem(int nmbVectors = 1) {                      // Problem_def.hpp:134-139
        system_.reset(new BlockMatrix_Type((UN)domainPtr_vec_.size()));
        initializeVectors(nmbVectors);
    }
    void initializeVectors(int nmbVectors = 1) {                      // Problem_def.hpp:332-360
        const UN size = (UN)domainPtr_vec_.size();
        solution_.reset(new BlockMultiVector_Type(size));
        rhs_.reset(new BlockMultiVector_Type(size));
        sourceTerm_.reset(new BlockMultiVector_Type(size));
        for (UN i = 0; i < size; ++i) {
            auto map = dofsPerNode_vec_[i] > 1 ? domainPtr_vec_[i]->getMapVecFieldUnique() : domainPtr_vec_[i]->getMapUnique();
            solution_->addBlock(Teuchos::rcp(new MultiVector_Type(map, nmbVectors)), i);
            rhs_->addBlock(Teuchos::rcp(new MultiVector_Type(map, nmbVectors)), i);
            sourceTerm_->addBlock(Teuchos::rcp(new MultiVector_Type(map, nmbVectors)), i);
        }
    }
    BlockMultiVectorPtr_Type getRhs() const { return rhs_; }
    BlockMultiVectorPtr_Type getSolution() { return solution_; }
    BlockMatrixPtr_Type getSystem() const { return system_; }
    bool getVerbose() const { return verbose_; }
    DomainConstPtr_Type getDomain(int i) const { return domainPtr_vec_.at(i); }
    std::string getFEType(int i) const { return domain_FEType_vec_.at(i); }
    std::string getVariableName(int i) const { return variableName_vec_.at(i); }
    int getDofsPerNode(int i) const { return dofsPerNode_vec_.at(i); }
    ParameterListPtr_Type getParameterList() const { return parameterList_; }
    void addToRhs(BlockMultiVectorPtr_Type x) const { rhs_->update(1., *x, 1.); }   // Problem_def.hpp:450-454
    BlockMultiVectorPtr_Type getSourceTerm() { return sourceTerm_; }
    CommConstPtr_Type getComm() const { return comm_; }
    void addParemeterRhs(double para) { parasSourceFunc_.push_back(para); }
    double getLastRelativeResidual() const { return lastRelativeResidual_; }
    BCConstPtr_Type getBCFactory() const { return bcFactory_; }      // what TimeProblem reads (fedd_time.hpp)
    // "Preconditioner Method" = "Diagonal" / "Triangular": the two child contexts (the reference's MinPrecProblems,
    // Preconditioner_def.hpp:979-1062), made by the first solve that asks for them and kept for the problem's life.  The
    // pressure mass matrix (Stokes_def.hpp:122-132, NavierStokes_def.hpp:177-183) is assembled in the Schur child, once.
    struct BlockPrecChildren {
        DeviceContextPtr velocity, schur;
        bool schurReady = false;
        fedd_ctx* parent = nullptr;
        ~BlockPrecChildren() { if (parent) fedd_block_prec_detach(parent); }
    };
    Teuchos::RCP<BlockPrecChildren>& blockPrecChildren() const { return blockPrec_; }
    FEFacPtr_Type getFEFactory() const { return feFactory_; }

    int dim_;
    mutable CommConstPtr_Type comm_;
    mutable BlockMatrixPtr_Type system_;
    mutable BlockMultiVectorPtr_Type rhs_;
    mutable BlockMultiVectorPtr_Type solution_;
    bool verbose_;
protected:
    mutable ParameterListPtr_Type parameterList_;
    mutable DomainConstPtr_vec_Type domainPtr_vec_;
    std::vector<std::string> domain_FEType_vec_, variableName_vec_;
    mutable BCConstPtr_Type bcFactory_;
    mutable Teuchos::RCP<BlockPrecChildren> blockPrec_;
    FEFacPtr_Type feFactory_;
    std::vector<int> dofsPerNode_vec_;
    mutable BlockMultiVectorPtr_Type sourceTerm_;
    std::vector<RhsFunc_Type> rhsFuncVec_;
    vec_dbl_Type parasSourceFunc_;
    double lastRelativeResidual_ = 0.;
    Teuchos::RCP<PrecOp_Type> userPrec_;
};

template <class SC, class LO, class GO, class NO>
int LinearSolver<SC, LO, GO, NO>::solve(Problem_Type* problem, BlockMultiVectorPtr_Type rhs, std::string type) {
    const bool constPrec = type.size() > 9 && type.compare(type.size() - 9, 9, "ConstPrec") == 0;
    const std::string method = constPrec ? type.substr(0, type.size() - 9) : type;
    const bool blockMethod = method == "Diagonal" || method == "Triangular";
    TEUCHOS_TEST_FOR_EXCEPTION(method != "Monolithic" && !blockMethod, std::logic_error,
                               "\"Preconditioner Method\" = \"" + type + "\" is not built (Monolithic, Diagonal and Triangular are, each also as ...ConstPrec; Teko and FaCSI are not)");
    auto system = problem->getSystem();
    const bool blocks = system->size() > 1;
    TEUCHOS_TEST_FOR_EXCEPTION(blocks && system->mergedDevice().is_null(), std::logic_error,
                               "block system: it has not been merged on the device (BlockMatrix::merge, done by the problem's assemble)");
    if (!blocks) TEUCHOS_TEST_FOR_EXCEPTION(!system->getBlock(0, 0)->isResident(), std::runtime_error, "solve: the system matrix is not resident on the device");
    fedd_ctx* ctx = blocks ? system->mergedDevice()->ctx : system->getBlock(0, 0)->device()->ctx;
    auto pl = problem->getParameterList();
    // same keys the reference's XML files use (laplace/parametersSolver.xml, parametersPrec.xml)
    auto& belos = pl->sublist("ThyraSolver").sublist("Linear Solver Types").sublist("Belos");
    const std::string solverType = belos.get("Solver Type", "Block GMRES");
    // Stratimikos hands the string to Belos; of its solvers "Block GMRES" (fedd_gmres) and "Block CG" / "Pseudo Block CG"
    // (fedd_cg, block size 1) are built.  Anything else is an error, not a GMRES run on an empty sublist
    const bool useCg = solverType == "Block CG" || solverType == "Pseudo Block CG";
    TEUCHOS_TEST_FOR_EXCEPTION(!useCg && solverType != "Block GMRES", std::logic_error,
                               "Solver Type \"" + solverType + "\" is not built (Block GMRES, Block CG, Pseudo Block CG are)");
    auto& gm = belos.sublist("Solver Types").sublist(solverType);
    const double tol = gm.get("Convergence Tolerance", 1e-8);
    const int maxIt = gm.get("Maximum Iterations", 100);
    const int numBlocks = gm.get("Num Blocks", 100);
    auto& frosch = pl->sublist("ThyraPreconditioner").sublist("Preconditioner Types").sublist("FROSch");
    const std::string precType = pl->sublist("ThyraPreconditioner").get("Preconditioner Type", "FROSch");
    const int cmb = combineMode(frosch);
    const bool usePrec = precType != "None" || blockMethod;
    // CG needs a symmetric preconditioner (the words of fedd_cg's own error)
    TEUCHOS_TEST_FOR_EXCEPTION(useCg && usePrec && problem->getUserPreconditioner().is_null() && cmb != FEDD_COMBINE_FULL, std::logic_error,
                               solverType + ": preconditioner not symmetric: use FEDD_COMBINE_FULL (\"Combine Values in Overlap\" = \"Full\")");
    TEUCHOS_TEST_FOR_EXCEPTION(useCg && !problem->getUserPreconditioner().is_null(), std::logic_error,
                               solverType + ": user preconditioner operators run with Block GMRES only");
    TEUCHOS_TEST_FOR_EXCEPTION(useCg && blocks, std::logic_error, solverType + ": a merged block system is not symmetric positive definite; use Block GMRES");
    if (blockMethod) {
        TEUCHOS_TEST_FOR_EXCEPTION(!blocks || system->size() != 2, std::logic_error,
                                   "\"Preconditioner Method\" = \"" + type + "\" needs a 2 x 2 block system (Stokes, NavierStokes)");
        TEUCHOS_TEST_FOR_EXCEPTION(!problem->getUserPreconditioner().is_null(), std::logic_error, type + ": not with a user preconditioner operator");
        if (!constPrec) setupBlockPreconditioner(problem, ctx, method);
        TEUCHOS_TEST_FOR_EXCEPTION(problem->blockPrecChildren().is_null(), std::logic_error, type + ": no preconditioner has been built yet to keep");
    } else {
        // a block preconditioner of an earlier solve does not outlive a change of method
        if (!problem->blockPrecChildren().is_null()) problem->blockPrecChildren() = Teuchos::null;
        if (usePrec && !constPrec) setupSchwarz(ctx, pl->sublist("ThyraPreconditioner"), *pl, blocks, problem->getVerbose());
    }
    auto b = rhs.is_null() ? problem->getRhs() : rhs;
    auto x = problem->getSolution();
    int its = 0;
    double rel = 0.;
    // "Zero Initial Guess" (LinearSolver_def.hpp:76-78): true clears the solution vector, false keeps it as x_0.
    // "Level Combination" = "Multiplicative" (:98-104): one coarse-only application of the preconditioner to the right-hand
    // side goes into the solution vector before the solve, which then starts from it (and runs the multiplicative
    // preconditioner set up above)
    const bool zeroGuess = pl->get("Zero Initial Guess", true);
    if (zeroGuess) x->putScalar(0.);
    const bool multiplicative = usePrec && !blockMethod && std::string(frosch.get("Level Combination", "Additive")) == "Multiplicative";
    TEUCHOS_TEST_FOR_EXCEPTION(multiplicative && (blocks || !frosch.get("TwoLevel", false)), std::logic_error,
                               "Level Combination = Multiplicative needs the coarse level (TwoLevel = true, single-block system)");
    if (!problem->getUserPreconditioner().is_null()) {
        // INTEGRATION.md 3(b), "keep the iterative solver, plug in operator and preconditioner": right-preconditioned
        // GMRES(m) on the host -- what Belos' Block GMRES does with Thyra operators (LinearSolver_def.hpp:72-135), two-pass
        // classical Gram-Schmidt like its ICGS manager -- with A = Matrix::apply (fedd_spmv) and M^-1 = the user's operator
        TEUCHOS_TEST_FOR_EXCEPTION(blocks, std::logic_error, "user preconditioner operators: single-block systems in this build");
        its = hostGmres(*system->getBlock(0, 0), *problem->getUserPreconditioner(), *b->getBlock(0), *x->getBlockNonConst(0), tol, maxIt,
                        numBlocks, rel);
        lastRelativeResidual = rel;
        return its;
    }
    if (useCg) {
        TEUCHOS_TEST_FOR_EXCEPTION(multiplicative, std::logic_error, solverType + ": FEDD_LEVELS_MULTIPLICATIVE is not symmetric: use \"Level Combination\" = \"Additive\"");
        if (!zeroGuess)
            feddCheck(fedd_cg_x0(ctx, b->getBlock(0)->raw().data(), x->getBlockNonConst(0)->raw().data(), tol, maxIt, usePrec ? 1 : 0, &its, &rel), "fedd_cg_x0");
        else
            feddCheck(fedd_cg(ctx, b->getBlock(0)->raw().data(), x->getBlockNonConst(0)->raw().data(), tol, maxIt, usePrec ? 1 : 0, &its, &rel), "fedd_cg");
    } else if (!blocks) {
        if (multiplicative && problem->getUserPreconditioner().is_null())
            feddCheck(fedd_schwarz_coarse_apply(ctx, b->getBlock(0)->raw().data(), x->getBlockNonConst(0)->raw().data()), "fedd_schwarz_coarse_apply");
        if (multiplicative || !zeroGuess)
            feddCheck(fedd_gmres_x0(ctx, b->getBlock(0)->raw().data(), x->getBlockNonConst(0)->raw().data(), tol, maxIt, numBlocks,
                                    usePrec ? 1 : 0, &its, &rel), "fedd_gmres_x0");
        else
            feddCheck(fedd_gmres(ctx, b->getBlock(0)->raw().data(), x->getBlockNonConst(0)->raw().data(), tol, maxIt, numBlocks,
                                 usePrec ? 1 : 0, &its, &rel), "fedd_gmres");
    } else {       // merged vectors = the blocks one after the other (BlockMap::merge, BlockMap_def.hpp:55-80)
        std::vector<double> bb, xx;
        for (UN k = 0; k < b->size(); ++k) bb.insert(bb.end(), b->getBlock(k)->raw().begin(), b->getBlock(k)->raw().end());
        xx.assign(bb.size(), 0.);
        feddCheck(fedd_gmres(ctx, bb.data(), xx.data(), tol, maxIt, numBlocks, usePrec ? 1 : 0, &its, &rel), "fedd_gmres");
        size_t off = 0;
        for (UN k = 0; k < x->size(); ++k) {
            auto& dst = x->getBlockNonConst(k)->raw();
            std::copy(xx.begin() + off, xx.begin() + off + dst.size(), dst.begin());
            off += dst.size();
        }
    }
    lastRelativeResidual = rel;
    return its;
}

template <class SC, class LO, class GO, class NO>
int LinearSolver<SC, LO, GO, NO>::combineMode(Teuchos::ParameterList& frosch) {
    auto& ovl = frosch.sublist("AlgebraicOverlappingOperator");
    std::string combine = ovl.get("Combine Values in Overlap", "");
    if (combine.empty()) combine = ovl.get("Overlapping Operator Combination", "Restricted");
    return combine == "Averaging" ? FEDD_COMBINE_AVERAGING : (combine == "Full" ? FEDD_COMBINE_FULL : FEDD_COMBINE_RESTRICTED);
}

template <class SC, class LO, class GO, class NO>
void LinearSolver<SC, LO, GO, NO>::setupSchwarz(fedd_ctx* ctx, Teuchos::ParameterList& thyraPrec, Teuchos::ParameterList& pl, bool blocks, bool verbose) {
    auto& frosch = thyraPrec.sublist("Preconditioner Types").sublist("FROSch");
    const int overlap = frosch.get("Overlap", 1);
    const int cmb = combineMode(frosch);
    // "TwoLevel" = true (parametersPrec.xml:17) switches the coarse level on.  The coarse space is
    // this library's lattice space, not FROSch's GDSW: say so.
    const bool twoLevel = frosch.get("TwoLevel", false);
    // "CoarseOperator Type" (parametersPrec.xml:23): GDSWCoarseOperator / RGDSWCoarseOperator -> the library's GDSW /
    // RGDSW level on the coarse lattice; "Q1" = lattice hat functions; anything else (IPOUHarmonicCoarseOperator, the
    // third value the reference's XML files list) is not built: an error, not a silent substitute
    const std::string coarseType = frosch.get("CoarseOperator Type", "GDSWCoarseOperator");
    const int coarseKind = coarseType == "Q1" ? FEDD_COARSE_Q1 : (coarseType == "RGDSWCoarseOperator" ? FEDD_COARSE_RGDSW : FEDD_COARSE_GDSW);
    TEUCHOS_TEST_FOR_EXCEPTION(twoLevel && coarseType != "GDSWCoarseOperator" && coarseType != "RGDSWCoarseOperator" && coarseType != "Q1",
                               std::logic_error, "CoarseOperator Type \"" + coarseType + "\" is not built (GDSWCoarseOperator, RGDSWCoarseOperator, Q1 are)");
    const int target = frosch.get("Subdomain Nodes", 0);   // 0 = the library's default (27 / dofs per node)
    feddCheck(fedd_schwarz_set_target(ctx, target, 1.0), "fedd_schwarz_set_target");
    feddCheck(fedd_schwarz_set_coarse(ctx, frosch.get("Coarse Cells", 0.0)), "fedd_schwarz_set_coarse");
    // merged block systems: monolithic one-level Schwarz on the large-subdomain path; the coarse level takes
    // node-interleaved systems only (said once)
    if (blocks && twoLevel && verbose)
        std::cout << "-- note: the coarse level is not built for merged block systems; running one level --" << std::endl;
    const bool two = twoLevel && !blocks;
    // rotations in the null space of the coarse space: "Rotations" of the coarse operator's block 1
    // (steadyLinElas/parametersPrec.xml:100), which FROSch can only build from the node coordinates the reference hands over
    // with "Use node lists" (Preconditioner_def.hpp:266, 353-381; default true).  The library ignores the switch for
    // scalar problems (a rotation needs dofs = dim).
    if (two && coarseKind != FEDD_COARSE_Q1) {
        const bool nodeLists = pl.get("Use node lists", true);
        const bool rotations = frosch.sublist(coarseType).sublist("Blocks").sublist("1").get("Rotations", false);
        feddCheck(fedd_set_option(ctx, "gdsw_rotations", nodeLists && rotations ? 1.0 : 0.0), "fedd_set_option(gdsw_rotations)");
    }
    feddCheck(fedd_schwarz_setup(ctx, overlap, cmb, two ? 1 : 0, two ? coarseKind : 0), "fedd_schwarz_setup");
    // "Level Combination" = "Multiplicative" (parametersPrec.xml:19): FROSch's TwoLevelPreconditioner combines the levels
    // in every apply of the solve, z = (I - Pc A) M1^-1 r; the coarse pre-apply below supplies the Pc b term
    const bool mult = two && std::string(frosch.get("Level Combination", "Additive")) == "Multiplicative";
    feddCheck(fedd_schwarz_set_level_combination(ctx, mult ? FEDD_LEVELS_MULTIPLICATIVE : FEDD_LEVELS_ADDITIVE),
              "fedd_schwarz_set_level_combination");
}

// Preconditioner::buildPreconditionerBlock2x2 (Preconditioner_def.hpp:979-1062): one Schwarz preconditioner on the velocity block
// getBlock(0,0) (slot 0 for Stokes, 4 for Navier-Stokes) with the velocity Dirichlet rows, one on (1 / nu) M_p -- the positive
// definite matrix; the sign of the reference's -(1 / nu) M_p is the schur_scale -1 of the attach --, each from its own sublist
// ("Velocity preconditioner", "Schur complement preconditioner": their "ThyraPreconditioner", with the "General" list merged
// in as :1003-1008 does).  The children are made once per problem; every call imports the velocity block again (values only
// when its pattern stands: the Newton loop) and sets the velocity child up again; the Schur child is built once and kept.
template <class SC, class LO, class GO, class NO>
void LinearSolver<SC, LO, GO, NO>::setupBlockPreconditioner(Problem_Type* problem, fedd_ctx* ctx, const std::string& method) {
    auto pl = problem->getParameterList();
    auto system = problem->getSystem();
    auto& kids = problem->blockPrecChildren();
    if (kids.is_null()) {
        kids = Teuchos::rcp(new typename Problem_Type::BlockPrecChildren());
        kids->velocity = Teuchos::rcp(new DeviceContext(problem->getDomain(0)->getComm()));
        kids->schur = Teuchos::rcp(new DeviceContext(problem->getDomain(1)->getComm()));
        problem->getDomain(0)->uploadMeshTo(kids->velocity);
        problem->getDomain(1)->uploadMeshTo(kids->schur);
    }
    auto sublistOf = [&](const char* name) -> Teuchos::ParameterList& {
        auto& sub = pl->sublist(name);
        sub.sublist("General").setParameters(pl->sublist("General"));
        return sub;
    };
    feddCheck(fedd_sync(ctx), "fedd_sync");
    // velocity: F = getBlock(0,0), its Dirichlet rows, its setup
    const int slotF = system->getBlock(0, 0)->slot();
    TEUCHOS_TEST_FOR_EXCEPTION(slotF < 0, std::logic_error, method + ": block (0,0) is not a stored block of the device");
    feddCheck(fedd_matrix_import(kids->velocity->ctx, ctx, slotF), "fedd_matrix_import");
    TEUCHOS_TEST_FOR_EXCEPTION(problem->getBCFactory().is_null(), std::runtime_error, "No boundary conditions added.");
    std::vector<int32_t> rows;
    std::vector<double> values;
    problem->getBCFactory()->dirichletRowsOfBlock(problem->getRhs(), 0, rows, values);
    std::fill(values.begin(), values.end(), 0.);
    feddCheck(fedd_dirichlet_rows(kids->velocity->ctx, (int64_t)rows.size(), rows.data(), values.data()), "fedd_dirichlet_rows");
    auto& velList = sublistOf("Velocity preconditioner");
    setupSchwarz(kids->velocity->ctx, velList.sublist("ThyraPreconditioner"), velList, false, problem->getVerbose());
    // Schur complement: (1 / nu) M_p on the pressure mesh
    if (!kids->schurReady) {
        const double viscosity = pl->sublist("Parameter").get("Viscosity", 1.);
        TEUCHOS_TEST_FOR_EXCEPTION(!(viscosity > 0.), std::logic_error, method + ": the pressure mass matrix is scaled by 1 / Viscosity, which must be positive");
        feddCheck(fedd_pattern_build(kids->schur->ctx, 1, FEDD_BLOCK_SCALAR, nullptr), "fedd_pattern_build");
        feddCheck(fedd_assemble(kids->schur->ctx, FEDD_FORM_MASS, nullptr), "fedd_assemble");
        feddCheck(fedd_matrix_scale(kids->schur->ctx, -1, 1. / viscosity), "fedd_matrix_scale");
        auto& schurList = sublistOf("Schur complement preconditioner");
        setupSchwarz(kids->schur->ctx, schurList.sublist("ThyraPreconditioner"), schurList, false, problem->getVerbose());
        kids->schurReady = true;
    }
    feddCheck(fedd_block_prec_attach(ctx, method == "Diagonal" ? FEDD_BLOCKPREC_DIAGONAL : FEDD_BLOCKPREC_TRIANGULAR, kids->velocity->ctx,
                                     kids->schur->ctx, -1., 2), "fedd_block_prec_attach");
    kids->parent = ctx;
    if (problem->getVerbose()) std::cout << "-- block preconditioner " << method << ": velocity block from slot " << slotF << " --" << std::endl;
}

// Laplace (feddlib/problems/specific/Laplace_def.hpp:16-60)
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Laplace : public Problem<SC, LO, GO, NO> {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    Laplace(const DomainConstPtr_Type& domain, std::string FEType, ParameterListPtr_Type parameterList, bool vectorLaplace = false)
        : Problem_Type(parameterList, domain->getComm()), vectorLaplace_(vectorLaplace) {
        this->addVariable(domain, FEType, "u", vectorLaplace ? (int)domain->getDimension() : 1);
        this->dim_ = (int)this->getDomain(0)->getDimension();
    }
    void info() override { this->infoProblem(); }
    void assemble(std::string type = "") const override {
        (void)type;
        if (this->verbose_) std::cout << "-- Assembly Laplace ... " << std::flush;
        MatrixPtr_Type A;
        if (vectorLaplace_) {
            A = Teuchos::rcp(new Matrix_Type(this->domainPtr_vec_.at(0)->getMapVecFieldUnique(), this->getDomain(0)->getApproxEntriesPerRow()));
            this->feFactory_->assemblyLaplaceVecField(this->dim_, this->domain_FEType_vec_.at(0), 2, A);
        } else {
            A = Teuchos::rcp(new Matrix_Type(this->domainPtr_vec_.at(0)->getMapUnique(), this->getDomain(0)->getApproxEntriesPerRow()));
            this->feFactory_->assemblyLaplace(this->dim_, this->domain_FEType_vec_.at(0), 2, A);
        }
        this->system_->addBlock(A, 0, 0);
        this->assembleSourceTerm(0.);
        this->addToRhs(this->sourceTerm_);
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
    MatrixPtr_Type getMassMatrix() const {
        MatrixPtr_Type A = Teuchos::rcp(new Matrix_Type(this->domainPtr_vec_.at(0)->getMapUnique(), this->getDomain(0)->getApproxEntriesPerRow()));
        this->feFactory_->assemblyMass(this->dim_, this->domain_FEType_vec_.at(0), "Scalar", A);
        return A;
    }
private:
    bool vectorLaplace_;
};

// LinElas (feddlib/problems/specific/LinElas_def.hpp:64-99): lambda, E from mu, nu at :76-77
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class LinElas : public Problem<SC, LO, GO, NO> {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    LinElas(const DomainConstPtr_Type& domain, std::string FEType, ParameterListPtr_Type parameterList)
        : Problem_Type(parameterList, domain->getComm()) {
        this->addVariable(domain, FEType, "d_s", (int)domain->getDimension());
        this->dim_ = (int)this->getDomain(0)->getDimension();
    }
    void info() override { this->infoProblem(); }
    void assemble(std::string type = "") const override {
        (void)type;
        if (this->verbose_) std::cout << "-- Assembly linear elasticity ... " << std::flush;
        const double mu = this->parameterList_->sublist("Parameter").get("Mu", 2.0e6);
        const double nu = this->parameterList_->sublist("Parameter").get("Poisson Ratio", 0.4);
        const double E = mu * 2. * (1. + nu);
        const double lambda = nu * E / ((1. + nu) * (1. - 2. * nu));
        MatrixPtr_Type K = Teuchos::rcp(new Matrix_Type(this->getDomain(0)->getMapVecFieldUnique(), this->getDomain(0)->getApproxEntriesPerRow()));
        this->feFactory_->assemblyLinElasXDim(this->dim_, this->getDomain(0)->getFEType(), K, lambda, mu);
        this->system_->addBlock(K, 0, 0);
        this->assembleSourceTerm(0.);
        this->addToRhs(this->sourceTerm_);
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
};

// Geometry (feddlib/problems/specific/Geometry_def.hpp:37-101): the extension of a boundary displacement into the fluid mesh,
// one variable d_f.  "Model" = "Elasticity": assemblyLinElasXDim with the reference's lambda from "Poisson Ratio" (default 0.3)
// and "Mu".  "Model" = "Laplace" (the reference's default when the key is absent): assemblyLaplaceXDim with HeuristicScaling and
// "Distance Laplace" (default 0.03), "Coefficient Laplace" (default 1000), the Laplacian scaled where the mean distance of an
// element's vertices to the FSI interface is small.  It needs the distances of Domain::identifyInterfaceParallelAndDistance; on a
// domain without them it is an error that names "Elasticity" and that call.
// HeuristicScaling (Geometry_def.hpp:24-34)
inline double HeuristicScaling(double* x, double* parameter) { return x[0] < parameter[0] ? parameter[1] : 1.0; }

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Geometry : public Problem<SC, LO, GO, NO> {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    Geometry(const DomainConstPtr_Type& domain, std::string FEType, ParameterListPtr_Type parameterList)
        : Problem_Type(parameterList, domain->getComm()) {
        this->addVariable(domain, FEType, "d_f", (int)domain->getDimension());
        this->dim_ = (int)this->getDomain(0)->getDimension();
    }
    void info() override { this->infoProblem(); }
    void assemble(std::string type = "") const override {
        (void)type;
        const std::string model = this->parameterList_->sublist("Parameter").get("Model", "Laplace");
        if (model == "Laplace") {
            TEUCHOS_TEST_FOR_EXCEPTION(!this->getDomain(0)->hasDistancesToInterface(), std::logic_error,
                                       "Geometry: \"Model\" = \"Laplace\" (also the default when the key is absent) scales the Laplacian by the distance to an FSI "
                                       "interface: it needs Domain::identifyInterfaceParallelAndDistance first; without an interface set \"Model\" to \"Elasticity\".");
            if (this->verbose_) std::cout << "-- Assembly Geometry (scaled Laplace)... " << std::flush;
            double parameter[2] = {this->parameterList_->sublist("Parameter").get("Distance Laplace", 0.03),
                                   this->parameterList_->sublist("Parameter").get("Coefficient Laplace", 1000.)};
            if (this->verbose_) std::cout << "\n    Distance Laplace = " << parameter[0] << "  coefficient Laplace = " << parameter[1] << " ... " << std::flush;
            MatrixPtr_Type H = Teuchos::rcp(new Matrix_Type(this->getDomain(0)->getMapVecFieldUnique(),
                                                            this->getDomain(0)->getDimension() * this->getDomain(0)->getApproxEntriesPerRow()));
            this->feFactory_->assemblyLaplaceXDim(this->dim_, this->getDomain(0)->getFEType(), H, HeuristicScaling, parameter);
            this->system_->addBlock(H, 0, 0);
            this->assembleSourceTerm(0.);
            this->addToRhs(this->sourceTerm_);
            if (this->verbose_) std::cout << "done -- " << std::endl;
            return;
        }
        TEUCHOS_TEST_FOR_EXCEPTION(model != "Elasticity", std::logic_error, "Unknown model for geometry.");
        if (this->verbose_) std::cout << "-- Assembly Geometry (linear elasticity)... " << std::flush;
        const double poissonRatio = this->parameterList_->sublist("Parameter").get("Poisson Ratio", 0.3);
        const double mu = this->parameterList_->sublist("Parameter").get("Mu", 2.0e+6);
        const double youngModulus = mu * 2. * (1 + poissonRatio);
        const double lambda = (poissonRatio * youngModulus) / ((1 + poissonRatio) * (1 - 2 * poissonRatio));
        MatrixPtr_Type H = Teuchos::rcp(new Matrix_Type(this->getDomain(0)->getMapVecFieldUnique(),
                                                        this->getDomain(0)->getDimension() * this->getDomain(0)->getApproxEntriesPerRow()));
        this->feFactory_->assemblyLinElasXDim(this->dim_, this->getDomain(0)->getFEType(), H, lambda, mu);
        this->system_->addBlock(H, 0, 0);
        this->assembleSourceTerm(0.);
        this->addToRhs(this->sourceTerm_);
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
};

// Stokes (feddlib/problems/specific/Stokes_def.hpp:26-138): A = nu * vector Laplacian, B and B^T = -div blocks; the
// velocity domain is the P2 mesh built from the pressure domain's P1 mesh (its first nodes are the pressure nodes).
// The blocks live in slots of the velocity domain's device context and are merged there at the end of assemble()
// (BlockMatrix::merge at solve time in the reference); getBlock(i, j) gives host views of the blocks as assembled.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class Stokes : public Problem<SC, LO, GO, NO> {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    typedef typename Problem_Type::BlockMatrix_Type BlockMatrix_Type;
    Stokes(const DomainConstPtr_Type& domainVelocity, std::string FETypeVelocity, const DomainConstPtr_Type& domainPressure,
           std::string FETypePressure, ParameterListPtr_Type parameterList)
        : Problem_Type(parameterList, domainVelocity->getComm()) {
        this->addVariable(domainVelocity, FETypeVelocity, "u", (int)domainVelocity->getDimension());
        this->addVariable(domainPressure, FETypePressure, "p", 1);
        this->dim_ = (int)this->getDomain(0)->getDimension();
    }
    void info() override { this->infoProblem(); }
    void assemble(std::string type = "") const override {
        (void)type;
        if (this->verbose_) std::cout << "-- Assembly ... " << std::flush;
        const double viscosity = this->parameterList_->sublist("Parameter").get("Viscosity", 1.);
        TEUCHOS_TEST_FOR_EXCEPTION(this->getFEType(1) != "P1", std::logic_error, "Stokes: P1 pressure in this build");
        auto domV = this->getDomain(0);
        auto dev = domV->device();
        MatrixPtr_Type A(new Matrix_Type(domV->getMapVecFieldUnique(), domV->getApproxEntriesPerRow()));
        MatrixPtr_Type BT(new Matrix_Type(domV->getMapVecFieldUnique(), this->getDomain(1)->getDimension() * this->getDomain(1)->getApproxEntriesPerRow()));
        auto pressureMap = this->getDomain(1)->getMapUnique();
        MatrixPtr_Type B(new Matrix_Type(pressureMap, domV->getDimension() * domV->getApproxEntriesPerRow()));
        if (this->verbose_) std::cout << " A ... " << std::flush;
        if (this->parameterList_->sublist("Parameter").get("Symmetric gradient", false)) {   // Stokes_def.hpp:69-70: block (0,0) is FULL
            int dummy[1] = {0};
            this->feFactory_->assemblyStress(this->dim_, this->domain_FEType_vec_.at(0), A, OneFunction, dummy, true);
        } else
            this->feFactory_->assemblyLaplaceVecField(this->dim_, this->domain_FEType_vec_.at(0), 2, A, true);
        A->resumeFill();
        feddCheck(fedd_matrix_scale(dev->ctx, -1, viscosity), "fedd_matrix_scale");        // A->scale(viscosity), Stokes_def.hpp:83
        feddCheck(fedd_matrix_store(dev->ctx, 0), "fedd_matrix_store");
        A->bindSlot(dev, 0);
        if (this->verbose_) std::cout << "B and B^T ... " << std::flush;
        this->feFactory_->assemblyDivAndDivT(this->dim_, this->getFEType(0), this->getFEType(1), 2, B, BT, domV->getMapVecFieldUnique(), pressureMap, true);
        B->resumeFill();
        BT->resumeFill();
        B->scale(-1.);
        BT->scale(-1.);
        A->fillComplete(domV->getMapVecFieldUnique(), domV->getMapVecFieldUnique());
        B->fillComplete(domV->getMapVecFieldUnique(), pressureMap);
        BT->fillComplete(pressureMap, domV->getMapVecFieldUnique());
        this->system_.reset(new BlockMatrix_Type(2));
        this->system_->addBlock(A, 0, 0);
        this->system_->addBlock(BT, 0, 1);
        this->system_->addBlock(B, 1, 0);
        int slotC = -1;
        if (this->getFEType(0) == "P1") {       // Stokes_def.hpp:98-105: P1/P1 needs the stabilisation block C = -1/nu * BD
            if (this->verbose_) std::cout << "C ... " << std::flush;
            MatrixPtr_Type C(new Matrix_Type(pressureMap, this->getDomain(1)->getApproxEntriesPerRow()));
            this->feFactory_->assemblyBDStabilization(this->dim_, "P1", C, true);
            C->resumeFill();
            feddCheck(fedd_matrix_scale(dev->ctx, -1, -1. / viscosity), "fedd_matrix_scale");   // C->scale(-1./viscosity)
            feddCheck(fedd_matrix_store(dev->ctx, 3), "fedd_matrix_store");
            C->bindSlot(dev, 3);
            C->fillComplete(pressureMap, pressureMap);
            this->system_->addBlock(C, 1, 1);
            slotC = 3;
        }
        // BlockMatrix::merge: system <- [A B^T; B C] on the device (C empty for P2/P1)
        feddCheck(fedd_block_merge(dev->ctx, 0, 2, 1, slotC), "fedd_block_merge");
        dev->generation++;
        this->system_->setMerged(dev);
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
};

// NonLinearProblem (feddlib/problems/abstract/NonLinearProblem_def.hpp:97-160): residual vector, its norm, and the update solve
// system * dx = residual, solution <- dx + previous solution.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class NonLinearProblem : public Problem<SC, LO, GO, NO> {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::BlockMultiVector_Type BlockMultiVector_Type;
    typedef typename Problem_Type::BlockMultiVectorPtr_Type BlockMultiVectorPtr_Type;
    typedef typename Problem_Type::MultiVector_Type MultiVector_Type;
    typedef typename Problem_Type::CommConstPtr_Type CommConstPtr_Type;
    NonLinearProblem(ParameterListPtr_Type parameterList, CommConstPtr_Type comm) : Problem_Type(parameterList, comm) {}
    virtual void reAssemble(std::string type) const = 0;
    virtual void calculateNonLinResidualVec(std::string type = "standard", double time = 0.) const = 0;
    void infoNonlinProblem() {
        if (this->verbose_)
            std::cout << "\t ### Nonlinear problem: Linearization " << this->parameterList_->sublist("General").get("Linearization", "FixedPoint")
                      << ", relNonLinTol " << this->parameterList_->sublist("Parameter").get("relNonLinTol", 1.0e-6) << std::endl;
    }
    void initializeProblem(int nmbVectors = 1) {                      // NonLinearProblem_def.hpp:60-76
        Problem_Type::initializeProblem(nmbVectors);
        residualVec_ = likeSolution(nmbVectors);
        previousSolution_ = likeSolution(nmbVectors);
    }
    double calculateResidualNorm() const {                            // :121-127
        double s = 0.;
        for (UN b = 0; b < residualVec_->size(); ++b)
            for (double v : residualVec_->getBlock(b)->raw()) s += v * v;
        return std::sqrt(s);
    }
    int solveUpdate() {                                               // :130-138
        previousSolution_->update(1., *this->solution_, 0.);
        return this->solve(residualVec_);
    }
    int solveAndUpdate(const std::string& criterion, double& criterionValue) {   // :141-154
        int its = solveUpdate();
        if (criterion == "Update") {
            double s = 0.;
            for (UN b = 0; b < this->solution_->size(); ++b)
                for (double v : this->solution_->getBlock(b)->raw()) s += v * v;
            criterionValue = std::sqrt(s);
        }
        this->solution_->update(1., *previousSolution_, 1.);
        return its;
    }
    BlockMultiVectorPtr_Type getResidualVector() const { return residualVec_; }
    void setBoundariesSystem() const {                                // Problem_def.hpp: BCBuilder::setSystem on the system alone
        TEUCHOS_TEST_FOR_EXCEPTION(this->bcFactory_.is_null(), std::runtime_error, "No boundary conditions added.");
        this->bcFactory_->setSystem(this->system_, this->rhs_);
    }
    void setBoundariesRHS(double time = .0) const {
        TEUCHOS_TEST_FOR_EXCEPTION(this->bcFactory_.is_null(), std::runtime_error, "No boundary conditions added.");
        this->bcFactory_->setRHS(this->rhs_, time);
    }
protected:
    BlockMultiVectorPtr_Type likeSolution(int nmbVectors) const {
        BlockMultiVectorPtr_Type v(new BlockMultiVector_Type(this->solution_->size()));
        for (UN i = 0; i < this->solution_->size(); ++i)
            v->addBlock(Teuchos::rcp(new MultiVector_Type(this->solution_->getBlock(i)->getMap(), nmbVectors)), i);
        return v;
    }
    mutable BlockMultiVectorPtr_Type residualVec_, previousSolution_;
};

// NavierStokes (feddlib/problems/specific/NavierStokes_def.hpp): A = density * viscosity * vector Laplacian, B and B^T = -div
// blocks, C = -1 / (viscosity density) BD for P1 / P1 (assembleConstantMatrices); per nonlinear iteration block (0,0) =
// A + density N(u) ("FixedPoint") or A + density (N(u) + W(u)) ("Newton"), reAssemble :282-321, from one device pass
// (fedd_assemble_advection) into slot 4, merged again with the constant blocks (values only after the first time).
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class NavierStokes : public NonLinearProblem<SC, LO, GO, NO> {
public:
    typedef NonLinearProblem<SC, LO, GO, NO> NonLinearProblem_Type;
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    typedef typename Problem_Type::BlockMatrix_Type BlockMatrix_Type;
    NavierStokes(const DomainConstPtr_Type& domainVelocity, std::string FETypeVelocity, const DomainConstPtr_Type& domainPressure,
                 std::string FETypePressure, ParameterListPtr_Type parameterList)
        : NonLinearProblem_Type(parameterList, domainVelocity->getComm()) {
        this->addVariable(domainVelocity, FETypeVelocity, "u", (int)domainVelocity->getDimension());
        this->addVariable(domainPressure, FETypePressure, "p", 1);
        this->dim_ = (int)this->getDomain(0)->getDimension();
    }
    void info() override { this->infoProblem(); this->infoNonlinProblem(); }
    void assemble(std::string type = "") const override {
        if (type == "") {
            if (this->verbose_) std::cout << "-- Assembly Navier-Stokes ... " << std::endl;
            assembleConstantMatrices();
            if (this->verbose_) std::cout << "done -- " << std::endl;
        } else {
            reAssemble(type);
        }
    }
    void assembleConstantMatrices() const {
        if (this->verbose_) std::cout << "-- Assembly constant matrices Navier-Stokes ... " << std::flush;
        auto& par = this->parameterList_->sublist("Parameter");
        const double viscosity = par.get("Viscosity", 1.), density = par.get("Density", 1.);
        TEUCHOS_TEST_FOR_EXCEPTION(par.get("Symmetric gradient", false), std::logic_error,
                                   "\"Symmetric gradient\" = true is refused by NavierStokes in this build: its velocity block is the vector Laplacian (set the key to false); of the flow problems Stokes assembles the stress form");
        TEUCHOS_TEST_FOR_EXCEPTION(this->getFEType(1) != "P1", std::logic_error, "NavierStokes: P1 pressure in this build");
        TEUCHOS_TEST_FOR_EXCEPTION(this->comm_->getSize() > 1, std::logic_error, "NavierStokes: one rank in this build");
        auto domV = this->getDomain(0);
        auto dev = domV->device();
        if (par.get("Set Zeros", false)) this->feFactory_->doSetZeros(par.get("Myeps", 1.0e-14));
        MatrixPtr_Type A(new Matrix_Type(domV->getMapVecFieldUnique(), domV->getApproxEntriesPerRow()));
        MatrixPtr_Type BT(new Matrix_Type(domV->getMapVecFieldUnique(), this->getDomain(1)->getDimension() * this->getDomain(1)->getApproxEntriesPerRow()));
        auto pressureMap = this->getDomain(1)->getMapUnique();
        MatrixPtr_Type B(new Matrix_Type(pressureMap, domV->getDimension() * domV->getApproxEntriesPerRow()));
        this->feFactory_->assemblyLaplaceVecField(this->dim_, this->domain_FEType_vec_.at(0), 2, A, true);
        A->resumeFill();
        feddCheck(fedd_matrix_scale(dev->ctx, -1, viscosity * density), "fedd_matrix_scale");   // A_->scale(viscosity); A_->scale(density)
        feddCheck(fedd_matrix_store(dev->ctx, 0), "fedd_matrix_store");
        A->bindSlot(dev, 0);
        this->feFactory_->assemblyDivAndDivT(this->dim_, this->getFEType(0), this->getFEType(1), 2, B, BT, domV->getMapVecFieldUnique(), pressureMap, true);
        B->resumeFill();
        BT->resumeFill();
        B->scale(-1.);
        BT->scale(-1.);
        A->fillComplete(domV->getMapVecFieldUnique(), domV->getMapVecFieldUnique());
        B->fillComplete(domV->getMapVecFieldUnique(), pressureMap);
        BT->fillComplete(pressureMap, domV->getMapVecFieldUnique());
        A_ = A;
        this->system_.reset(new BlockMatrix_Type(2));
        this->system_->addBlock(BT, 0, 1);
        this->system_->addBlock(B, 1, 0);
        slotC_ = -1;
        if (this->getFEType(0) == "P1") {
            MatrixPtr_Type C(new Matrix_Type(pressureMap, this->getDomain(1)->getApproxEntriesPerRow()));
            this->feFactory_->assemblyBDStabilization(this->dim_, "P1", C, true);
            C->resumeFill();
            feddCheck(fedd_matrix_scale(dev->ctx, -1, -1. / (viscosity * density)), "fedd_matrix_scale");
            feddCheck(fedd_matrix_store(dev->ctx, 3), "fedd_matrix_store");
            C->bindSlot(dev, 3);
            C->fillComplete(pressureMap, pressureMap);
            this->system_->addBlock(C, 1, 1);
            slotC_ = 3;
        }
        if (this->verbose_) std::cout << "done -- " << std::endl;
        reAssemble("FixedPoint");      // block (0,0) = A + density N(u) for the initial (zero) velocity, and the merged system
    }
    void reAssemble(std::string type) const override {
        if (this->verbose_) std::cout << "-- Reassembly Navier-Stokes (" << type << ") ... " << std::flush;
        TEUCHOS_TEST_FOR_EXCEPTION(type != "FixedPoint" && type != "Newton", std::logic_error, "reAssemble: unknown type " + type);
        const double density = this->parameterList_->sublist("Parameter").get("Density", 1.);
        auto domV = this->getDomain(0);
        auto dev = domV->device();
        // after a residual with mesh velocity (calculateNonLinResidualVecWithMeshVelo) the Newton matrix is that of the ALE block,
        // FSI_def.hpp:533-541; a "FixedPoint" call is the fixed-mesh one and needs clearMeshVelocity() first
        TEUCHOS_TEST_FOR_EXCEPTION(aleActive_ && type == "FixedPoint", std::logic_error,
                                   "reAssemble(\"FixedPoint\") with a mesh velocity in force: what is built is reAssembleFSI(\"FixedPoint\", u_minus_w, P) "
                                   "for the ALE block, or clearMeshVelocity() and then the fixed-mesh block");
        if (type == "FixedPoint") {     // u_rep_->importFromVector(u): the "Newton" call that follows keeps this velocity
            importVelocity();
            feddCheck(fedd_velocity_set(dev->ctx, u_rep_.data()), "fedd_velocity_set");
        }
        if (aleActive_) feddCheck(fedd_assemble_advection_ale(dev->ctx, FEDD_ALE_NEWTON, density, baseSlot_, 4), "fedd_assemble_advection_ale");
        else feddCheck(fedd_assemble_advection(dev->ctx, type == "Newton" ? FEDD_ADV_NEWTON : FEDD_ADV_N, density, baseSlot_, 4), "fedd_assemble_advection");
        finishVelocityBlock();
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
    // block (0,0) <- slot 4, merged with the constant blocks (values only after the first time)
    void finishVelocityBlock() const {
        auto domV = this->getDomain(0);
        auto dev = domV->device();
        MatrixPtr_Type ANW(new Matrix_Type(domV->getMapVecFieldUnique(), domV->getDimension() * domV->getApproxEntriesPerRow()));
        ANW->bindSlot(dev, 4);
        ANW->fillComplete(domV->getMapVecFieldUnique(), domV->getMapVecFieldUnique());
        this->system_->addBlock(ANW, 0, 0);
        feddCheck(fedd_block_merge(dev->ctx, 4, 2, 1, slotC_), "fedd_block_merge");
        dev->generation++;
        this->system_->setMerged(dev);
    }
    // u_rep_->importFromVector(u) (NavierStokes_def.hpp:251, 290)
    void importVelocity() const {
        auto domV = this->getDomain(0);
        auto mapRep = domV->getMapRepeated();
        auto mapUni = domV->getMapUnique();
        const auto& u = this->solution_->getBlock(0)->raw();
        const int dim = this->dim_;
        u_rep_.assign((size_t)mapRep->getNodeNumElements() * dim, 0.);
        for (LO i = 0; i < mapRep->getNodeNumElements(); ++i) {
            const LO k = mapUni->getLocalElement(mapRep->getGlobalElement(i));
            for (int d = 0; d < dim; ++d) u_rep_[(size_t)i * dim + d] = u[(size_t)k * dim + d];
        }
    }
    // NavierStokes::reAssembleFSI (NavierStokes_def.hpp:245-278): block (0,0) = A + density N(u - w) + P, P = -density P(w) given
    // by the caller (FSI_def.hpp:497-503).  The device forms u - w and -density P(w) itself from u_rep_ and the mesh velocity in
    // force (FEDD_ALE_FIXEDPOINT, scale = density, one pass), so the two arguments are CHECKED, not used: P must be the matrix
    // FE::assemblyAdditionalConvection returned last on this context, scaled by exactly -density, and u_minus_w must equal
    // u_rep_ - w entry by entry.
    void reAssembleFSI(std::string type, Teuchos::RCP<MultiVector<SC, LO, GO, NO> > u_minus_w, MatrixPtr_Type P) const {
        if (this->verbose_) std::cout << "-- Reassembly Navier-Stokes (FSI) ... " << std::flush;
        TEUCHOS_TEST_FOR_EXCEPTION(type != "FixedPoint", std::logic_error, "Newton method not implemented in reAssembleFSI.");
        const double density = this->parameterList_->sublist("Parameter").get("Density", 1.);
        auto domV = this->getDomain(0);
        auto dev = domV->device();
        TEUCHOS_TEST_FOR_EXCEPTION(P.is_null() || u_minus_w.is_null(), std::runtime_error, "reAssembleFSI: P or u_minus_w is null.");
        TEUCHOS_TEST_FOR_EXCEPTION(P->device().is_null() || P->device()->ctx != dev->ctx || P->additionalConvectionSerial() == 0 || P->additionalConvectionSerial() != dev->aleSerial,
                                   std::logic_error, "reAssembleFSI: P is not the matrix FE::assemblyAdditionalConvection returned last on this domain; what is built is "
                                   "A + density N(u - w) - density P(w) for the mesh velocity in force, formed on the device");
        TEUCHOS_TEST_FOR_EXCEPTION(P->additionalConvectionScale() != -density, std::logic_error,
                                   "reAssembleFSI: P is scaled by " << P->additionalConvectionScale() << " and must be scaled by exactly -density = " << -density
                                   << " (P->scale(density); P->scale(-1.0), FSI_def.hpp:501-503); what is built is A + density N(u - w) - density P(w)");
        importVelocity();
        std::vector<double> w(u_rep_.size());
        feddCheck(fedd_mesh_velocity_get(dev->ctx, w.data()), "fedd_mesh_velocity_get");
        const auto& c = u_minus_w->raw(0);
        TEUCHOS_TEST_FOR_EXCEPTION(c.size() != u_rep_.size(), std::logic_error, "reAssembleFSI: u_minus_w does not live on the repeated vector-field map");
        for (size_t i = 0; i < c.size(); ++i)
            TEUCHOS_TEST_FOR_EXCEPTION(c[i] != u_rep_[i] - w[i], std::logic_error,
                                       "reAssembleFSI: u_minus_w is not u - w (entry " << i << ": " << c[i] << " against " << u_rep_[i] - w[i]
                                       << "); what is built convects by the solution's velocity minus the mesh velocity in force");
        feddCheck(fedd_velocity_set(dev->ctx, u_rep_.data()), "fedd_velocity_set");
        feddCheck(fedd_assemble_advection_ale(dev->ctx, FEDD_ALE_FIXEDPOINT, density, baseSlot_, 4), "fedd_assemble_advection_ale");
        aleActive_ = true;
        finishVelocityBlock();
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
    // NavierStokes_def.hpp:754-760, then the residual of calculateNonLinResidualVec
    void calculateNonLinResidualVecWithMeshVelo(std::string type, double time, Teuchos::RCP<MultiVector<SC, LO, GO, NO> > u_minus_w, MatrixPtr_Type P) const {
        reAssembleFSI("FixedPoint", u_minus_w, P);
        residualOfTheSystem(type, time);
    }
    // facade only: back to the fixed-mesh path
    void clearMeshVelocity() const {
        feddCheck(fedd_mesh_velocity_set(this->getDomain(0)->device()->ctx, nullptr), "fedd_mesh_velocity_set");
        aleActive_ = false;
    }
    // NavierStokes_def.hpp:723-751: residual = system(u) x - rhs ("standard") or rhs - system(u) x ("reverse"), the Dirichlet
    // rows x - g / g - x
    void calculateNonLinResidualVec(std::string type = "standard", double time = 0.) const override {
        reAssemble("FixedPoint");
        residualOfTheSystem(type, time);
    }
    void residualOfTheSystem(std::string type, double time) const {
        auto dev = this->getDomain(0)->device();
        std::vector<double> x, y;
        for (UN b = 0; b < this->solution_->size(); ++b)
            x.insert(x.end(), this->solution_->getBlock(b)->raw().begin(), this->solution_->getBlock(b)->raw().end());
        y.assign(x.size(), 0.);
        feddCheck(fedd_spmv(dev->ctx, x.data(), y.data()), "fedd_spmv");
        size_t off = 0;
        const bool standard = type == "standard";
        TEUCHOS_TEST_FOR_EXCEPTION(!standard && type != "reverse", std::logic_error, "calculateNonLinResidualVec: unknown type " + type);
        for (UN b = 0; b < this->residualVec_->size(); ++b) {
            auto& r = this->residualVec_->getBlockNonConst(b)->raw();
            const auto& f = this->rhs_->getBlock(b)->raw();
            for (size_t i = 0; i < r.size(); ++i) r[i] = standard ? y[off + i] - f[i] : f[i] - y[off + i];
            off += r.size();
        }
        if (standard) this->bcFactory_->setVectorMinusBC(this->residualVec_, this->solution_, time);
        else this->bcFactory_->setBCMinusVector(this->residualVec_, this->solution_, time);
    }
    // the slot reAssemble hands to fedd_assemble_advection as slot_add: 0 = A (steady); a time loop sets 6, the time-combined
    // constant block (cm M) + (ca A) (TimeProblem::combineSystems, fedd_time.hpp)
    void setVelocityBaseSlot(int slot) const { baseSlot_ = slot; }
    int getVelocityBaseSlot() const { return baseSlot_; }
private:
    mutable MatrixPtr_Type A_;
    mutable std::vector<double> u_rep_;
    mutable int slotC_ = -1, baseSlot_ = 0;
    mutable bool aleActive_ = false;   // the last residual was one with mesh velocity: reAssemble("Newton") builds the ALE Newton block
};

// NonLinElasticity (feddlib/problems/specific/NonLinElasticity_def.hpp:16-120, 251-271): one vector block; every
// "Newton-Residual" reassembly is one device pass (fedd_assemble_hyperelastic) for the tangent, which becomes the system matrix,
// and the internal force, which becomes the residual vector.  "Newton" is a no-op, as in the reference (:112-117).
// The source term enters twice, as in the reference: assemble("") adds it to rhs_ (:61-62) and calculateNonLinResidualVec
// subtracts rhs_ AND sourceTerm_ (:254-263), so the residual is f(u) - 2 * source on the free rows.  Restated, not corrected.
// Per-flag materials ("E1" / "E2" / "Mu1" / "Mu2" on elements flagged 1 / 2, FE_def.hpp:1164-1174) are not built: an error
// where such elements exist and the parameter differs from the base one.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class NonLinElasticity : public NonLinearProblem<SC, LO, GO, NO> {
public:
    typedef NonLinearProblem<SC, LO, GO, NO> NonLinearProblem_Type;
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::DomainConstPtr_Type DomainConstPtr_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    typedef typename Problem_Type::BlockMatrix_Type BlockMatrix_Type;
    typedef typename Problem_Type::BlockMultiVectorPtr_Type BlockMultiVectorPtr_Type;
    NonLinElasticity(const DomainConstPtr_Type& domain, std::string FEType, ParameterListPtr_Type parameterList)
        : NonLinearProblem_Type(parameterList, domain->getComm()) {
        this->addVariable(domain, FEType, "u", (int)domain->getDimension());
        this->dim_ = (int)this->getDomain(0)->getDimension();
        C_ = this->parameterList_->sublist("Parameter").get("C", 1.);
    }
    void info() override { this->infoProblem(); this->infoNonlinProblem(); }
    void assemble(std::string type = "") const override {
        if (type != "") { reAssemble(type); return; }
        if (this->verbose_) std::cout << "-- Assembly nonlinear elasticity ... " << std::flush;
        TEUCHOS_TEST_FOR_EXCEPTION(this->comm_->getSize() > 1, std::logic_error, "NonLinElasticity: one rank in this build");
        auto dom = this->getDomain(0);
        auto dev = dom->device();
        int64_t nnz = 0;
        feddCheck(fedd_pattern_build(dev->ctx, this->dim_, FEDD_BLOCK_FULL, &nnz), "fedd_pattern_build");   // assemblyEmptyMatrix
        dev->generation++;
        MatrixPtr_Type A(new Matrix_Type(dom->getMapVecFieldUnique(), dom->getDimension() * dom->getApproxEntriesPerRow()));
        A->bind(dev, this->dim_);
        this->system_.reset(new BlockMatrix_Type(1));
        this->system_->addBlock(A, 0, 0);
        this->assembleSourceTerm(0.);
        this->addToRhs(this->sourceTerm_);
        this->setBoundariesRHS();
        this->solution_->putScalar(0.);
        if (this->verbose_) std::cout << "done -- " << std::endl;
        reAssemble("Newton-Residual");
    }
    void reAssemble(std::string type) const override {
        auto& par = this->parameterList_->sublist("Parameter");
        const std::string model = par.get("Material model", "Neo-Hooke");
        if (this->verbose_) std::cout << "-- Reassembly nonlinear elasticity with material model " << model << " (" << type << ") ... " << std::flush;
        if (type == "Newton-Residual") {
            auto dom = this->getDomain(0);
            auto dev = dom->device();
            const int dim = this->dim_;
            double p[3];
            int np = 0;
            const int id = material(p, np);
            // u_rep_->importFromVector(u)
            auto mapRep = dom->getMapRepeated();
            auto mapUni = dom->getMapUnique();
            const auto& u = this->solution_->getBlock(0)->raw();
            u_rep_.assign((size_t)mapRep->getNodeNumElements() * dim, 0.);
            for (LO i = 0; i < mapRep->getNodeNumElements(); ++i) {
                const LO k = mapUni->getLocalElement(mapRep->getGlobalElement(i));
                for (int d = 0; d < dim; ++d) u_rep_[(size_t)i * dim + d] = u[(size_t)k * dim + d];
            }
            feddCheck(fedd_velocity_set(dev->ctx, u_rep_.data()), "fedd_velocity_set");
            feddCheck(fedd_assemble_hyperelastic(dev->ctx, id, p, np, FEDD_HYPER_TANGENT | FEDD_HYPER_FORCE), "fedd_assemble_hyperelastic");
            feddCheck(fedd_hyperelastic_force_get(dev->ctx, this->residualVec_->getBlockNonConst(0)->raw().data()), "fedd_hyperelastic_force_get");
            dev->generation++;
            MatrixPtr_Type W(new Matrix_Type(dom->getMapVecFieldUnique(), dom->getDimension() * dom->getApproxEntriesPerRow()));
            W->bind(dev, dim);
            this->system_->addBlock(W, 0, 0);
        } else {
            TEUCHOS_TEST_FOR_EXCEPTION(type != "Newton", std::logic_error, "NonLinElasticity::reAssemble: unknown type " + type + " (Newton-Residual and Newton are built)");
        }
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
    // the material of the parameter list as fedd_assemble_hyperelastic* takes it: the model id, its parameters and their number
    int material(double p[3], int& np) const {
        auto& par = this->parameterList_->sublist("Parameter");
        const std::string model = par.get("Material model", "Neo-Hooke");
        auto dom = this->getDomain(0);
        const int dim = this->dim_;
        const double nu = par.get("Poisson Ratio", 0.4), mu = par.get("Mu", 2.0e+6);
        const bool stvk = model == "Saint Venant-Kirchhoff";
        TEUCHOS_TEST_FOR_EXCEPTION(!stvk && model != "Neo-Hooke" && model != "Mooney-Rivlin", std::logic_error,
                                   "Material model \"" + model + "\" is not built (Neo-Hooke, Mooney-Rivlin, Saint Venant-Kirchhoff are)");
        TEUCHOS_TEST_FOR_EXCEPTION(dim == 2 && !stvk, std::logic_error, "Only Saint Venant-Kirchhoff in 2D.");
        const double E = stvk ? mu * 2. * (1. + nu) : par.get("E", 3.0e+6);     // FE_def.hpp:883-891
        for (int32_t flag : dom->elementFlags()) {
            if (flag != 1 && flag != 2) continue;
            const std::string base = stvk ? "Mu" : "E", key = base + (flag == 1 ? "1" : "2");
            const double other = par.get(key, stvk ? 2.0e+6 : 3.0e+6);
            TEUCHOS_TEST_FOR_EXCEPTION(other != (stvk ? mu : E), std::logic_error,
                                       "NonLinElasticity: the mesh has elements with flag " + std::to_string(flag) + " and \"" + key +
                                       "\" differs from \"" + base + "\": per-flag materials are not built (one material per assembly is)");
        }
        p[0] = E; p[1] = nu; p[2] = C_;
        np = model == "Mooney-Rivlin" ? 3 : 2;
        if (stvk) { p[0] = (nu * E) / ((1 + nu) * (1 - 2 * nu)); p[1] = mu; }   // lambda, mue (:894)
        return model == "Neo-Hooke" ? FEDD_HYPER_NEOHOOKE : (stvk ? FEDD_HYPER_STVK : FEDD_HYPER_MOONEY_RIVLIN);
    }
    // the system slot holds the FULL pattern again (after TimeProblem::assembleMassSystem used it for the mass matrix)
    void restorePattern() const {
        auto dom = this->getDomain(0);
        auto dev = dom->device();
        int64_t nnz = 0;
        feddCheck(fedd_pattern_build(dev->ctx, this->dim_, FEDD_BLOCK_FULL, &nnz), "fedd_pattern_build");
        rebind();
    }
    // the time tangent (cm M[slotMass]) + K(u) and the force for the displacement the DEVICE holds (fedd_newton_begin /
    // fedd_newton_update wrote the nodal vector field): one pass, nothing read back (TimeProblem, fedd_time.hpp)
    void reAssembleTime(int slotMass, double cm) const {
        double p[3];
        int np = 0;
        const int id = material(p, np);
        if (this->verbose_) std::cout << "-- Reassembly nonlinear elasticity, time tangent ... " << std::flush;
        feddCheck(fedd_assemble_hyperelastic_time(this->getDomain(0)->device()->ctx, id, p, np, FEDD_HYPER_TANGENT | FEDD_HYPER_FORCE, slotMass, cm),
                  "fedd_assemble_hyperelastic_time");
        rebind();
        if (this->verbose_) std::cout << "done -- " << std::endl;
    }
    void reAssembleExtrapolation(std::vector<BlockMultiVectorPtr_Type> previousSolutions) {
        (void)previousSolutions;
        TEUCHOS_TEST_FOR_EXCEPTION(true, std::logic_error, "Only Newton implemented for nonlinear material models! (NOX and extrapolation are not built)");
    }
    void calculateNonLinResidualVec(std::string type = "standard", double time = 0.) const override {
        reAssemble("Newton-Residual");
        const bool standard = type == "standard";
        TEUCHOS_TEST_FOR_EXCEPTION(!standard && type != "reverse", std::runtime_error, "Unknown type for residual computation.");
        auto& r = this->residualVec_->getBlockNonConst(0)->raw();
        const auto& f = this->rhs_->getBlock(0)->raw();
        const auto& s = this->sourceTerm_->getBlock(0)->raw();
        // :254-263: standard r <- r - rhs - source; reverse r <- rhs - r + source
        for (size_t i = 0; i < r.size(); ++i) r[i] = standard ? (r[i] - f[i]) - s[i] : (f[i] - r[i]) + s[i];
        this->bcFactory_->setBCMinusVector(this->residualVec_, this->solution_, time);
    }
private:
    void rebind() const {       // the system block follows the device's generation
        auto dom = this->getDomain(0);
        auto dev = dom->device();
        dev->generation++;
        MatrixPtr_Type W(new Matrix_Type(dom->getMapVecFieldUnique(), dom->getDimension() * dom->getApproxEntriesPerRow()));
        W->bind(dev, this->dim_);
        this->system_->addBlock(W, 0, 0);
    }
    mutable std::vector<double> u_rep_;
    double C_;
};

// NonLinearSolver (feddlib/problems/Solver/NonLinearSolver_def.hpp:274-391): solveFixedPoint and solveNewton, line by line --
// residual first ("reverse"), "Criterion" = Residual | Update, relNonLinTol, MaxNonLinIts, "Cancel MaxNonLinIts".  What the
// reference's parameter files can ask for beyond that is refused with the key named.
template <class SC, class LO, class GO, class NO>
class TimeProblem;      // fedd_time.hpp

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class NonLinearSolver {
public:
    typedef NonLinearProblem<SC, LO, GO, NO> NonLinearProblem_Type;
    typedef TimeProblem<SC, LO, GO, NO> TimeProblem_Type;
    // the TimeProblem overloads of NonLinearSolver_def.hpp (solveFixedPoint :394-452, solveNewton :459-531); defined in
    // fedd_time.hpp, which a caller of this overload includes anyway (DAESolverInTime)
    void solve(TimeProblem_Type& problem, double time);
    int lastNonLinIts = 0;          // nonlinear iterations of the last time-problem solve
    NonLinearSolver() : type_("") {}
    NonLinearSolver(std::string type) : type_(type) {}
    void solve(NonLinearProblem_Type& problem) {
        auto pl = problem.getParameterList();
        TEUCHOS_TEST_FOR_EXCEPTION(type_ == "NOX", std::logic_error, "\"Linearization\" = \"NOX\" is not built (FixedPoint and Newton are)");
        TEUCHOS_TEST_FOR_EXCEPTION(type_ != "FixedPoint" && type_ != "Newton", std::logic_error,
                                   "\"Linearization\" = \"" + type_ + "\" is not built (FixedPoint and Newton are)");
        const std::string prec = pl->sublist("General").get("Preconditioner Method", "Monolithic");
        TEUCHOS_TEST_FOR_EXCEPTION(prec != "Monolithic" && prec != "Diagonal" && prec != "Triangular", std::logic_error,
                                   "\"Preconditioner Method\" = \"" + prec + "\" is not built (Monolithic, Diagonal and Triangular are; Teko and FaCSI are not)");
        TEUCHOS_TEST_FOR_EXCEPTION(pl->sublist("Parameter").get("Symmetric gradient", false), std::logic_error,
                                   "\"Symmetric gradient\" = true is refused by the nonlinear problems of this build: their velocity block is the vector Laplacian (set the key to false); of the flow problems Stokes assembles the stress form");
        const std::string levels = pl->sublist("ThyraPreconditioner").sublist("Preconditioner Types").sublist("FROSch").get("Level Combination", "Additive");
        TEUCHOS_TEST_FOR_EXCEPTION(levels == "Multiplicative", std::logic_error,
                                   "\"Level Combination\" = \"Multiplicative\" is not supported for nonlinear problems (NonLinearProblem_def.hpp:578)");
        iterate(problem, type_ == "Newton");
    }
private:
    void iterate(NonLinearProblem_Type& problem, bool newton) {
        const bool verbose = problem.getVerbose();
        TEUCHOS_TEST_FOR_EXCEPTION(problem.getRhs()->getNumVectors() != 1, std::logic_error, "We need to change the code for numVectors>1.");
        const char* name = newton ? "Newton" : "Fixed Point";
        double gmresIts = 0., residual0 = 1., residual = 1.;
        auto& par = problem.getParameterList()->sublist("Parameter");
        const double tol = par.get("relNonLinTol", 1.0e-6);
        const int maxNonLinIts = par.get("MaxNonLinIts", 10);
        int nlIts = 0;
        double criterionValue = 1.;
        const std::string criterion = par.get("Criterion", "Residual");
        while (nlIts < maxNonLinIts) {
            problem.calculateNonLinResidualVec("reverse");
            if (newton) {
                if (criterion == "Residual") residual = problem.calculateResidualNorm();
                problem.assemble("Newton");
                problem.setBoundariesSystem();
            } else {
                problem.setBoundariesSystem();
                if (criterion == "Residual") residual = problem.calculateResidualNorm();
            }
            if (nlIts == 0) residual0 = residual;
            if (criterion == "Residual") {
                criterionValue = residual / residual0;
                if (verbose) std::cout << "### " << name << " iteration : " << nlIts << "  relative nonlinear residual : " << criterionValue << std::endl;
                if (criterionValue < tol) break;
            }
            gmresIts += problem.solveAndUpdate(criterion, criterionValue);
            nlIts++;
            if (criterion == "Update") {
                if (verbose) std::cout << "### " << name << " iteration : " << nlIts << "  residual of update : " << criterionValue << std::endl;
                if (criterionValue < tol) break;
            }
        }
        gmresIts /= std::max(nlIts, 1);
        if (verbose)
            std::cout << "### Total " << (newton ? "Newton iterations" : "FPI") << " : " << nlIts << "  with average gmres its : " << gmresIts << std::endl;
        if (par.get("Cancel MaxNonLinIts", false))
            TEUCHOS_TEST_FOR_EXCEPTION(nlIts == maxNonLinIts, std::runtime_error,
                                       "Maximum nonlinear Iterations reached. Problem might have converged in the last step. Still we cancel here.");
    }
    std::string type_;
};

// MeshPartitioner (feddlib/core/Mesh/MeshPartitioner_decl.hpp): reads the mesh named by "Mesh 1 Name" into the domain;
// on one rank no partitioning happens (MeshPartitioner_def.hpp:321-331).  The partitioner itself is in the library
// (fedd_mesh_partition*); the facade is one rank.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class MeshPartitioner {
public:
    typedef Domain<SC, LO, GO, NO> Domain_Type;
    typedef Teuchos::RCP<Domain_Type> DomainPtr_Type;
    typedef std::vector<DomainPtr_Type> DomainPtrArray_Type;
    MeshPartitioner(DomainPtrArray_Type domains, ParameterListPtr_Type pL, std::string feType, int dimension)
        : domains_(domains), pList_(pL), feType_(feType), dim_(dimension) {}
    void readAndPartition(int volumeID = 10) {
        for (size_t i = 0; i < domains_.size(); ++i) {
            const std::string name = pList_->get("Mesh " + std::to_string(i + 1) + " Name", std::string("noName"));
            domains_[i]->readMeshFile(name, dim_, feType_, volumeID);
        }
    }
private:
    DomainPtrArray_Type domains_;
    ParameterListPtr_Type pList_;
    std::string feType_;
    int dim_;
};

// ExporterParaView (feddlib/core/General/ExporterParaView_decl.hpp:45-175, _def.hpp:484-601): nodal fields of the
// unique map over the mesh, as an XDMF file ParaView opens.  The reference writes the heavy data through EpetraExt::HDF5;
// HDF5 is not available here, so the DataItems use XDMF's raw binary format (little endian): <name>.xmf plus
// <name>.conn.bin / <name>.xyz.bin / <name>.<variable>.<step>.bin.  One rank (the facade's scope); P2 meshes are written
// with their vertex connectivity (mid-edge nodes stay in the point list).
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class ExporterParaView {
public:
    typedef Domain<SC, LO, GO, NO> Mesh_Type;
    typedef Teuchos::RCP<const Mesh_Type> MeshPtr_Type;
    typedef MultiVector<SC, LO, GO, NO> MultiVec_Type;
    typedef Teuchos::RCP<const MultiVec_Type> MultiVecConstPtr_Type;
    typedef Map<LO, GO, NO> Map_Type;
    typedef Teuchos::RCP<const Map_Type> MapConstPtr_Type;

    ExporterParaView() {}
    void setup(std::string filename, MeshPtr_Type mesh, std::string FEType, ParameterListPtr_Type parameterList = Teuchos::null) {
        setup(filename, mesh, FEType, 1, parameterList);
    }
    // The exported arrays are GLOBAL arrays in files of their own, as in the reference's HDF5 file (ExporterParaView_def.hpp:
    // 484-601: every rank writes its hyperslab): points and nodal values in global-id order, the connectivity in global ids.
    // Rank 0 creates each file at its final size, then every rank writes its entries in place -- its unique nodes at
    // position gid, the elements it exports (those whose vertex of smallest global id it owns: exactly one rank per element,
    // and that rank holds the element among its own or ghost elements) behind those of the lower ranks.  The files do not
    // depend on the number of ranks.
    void setup(std::string filename, MeshPtr_Type mesh, std::string FEType, int saveTimestep, ParameterListPtr_Type = Teuchos::null) {
        TEUCHOS_TEST_FOR_EXCEPTION(mesh.is_null(), std::runtime_error, "ExporterParaView::setup: null mesh");
        filename_ = filename; mesh_ = mesh; FEType_ = FEType; saveTimestep_ = std::max(1, saveTimestep);
        comm_ = mesh->getComm();
        const int size = comm_->getSize(), rank = comm_->getRank();
        const int dim = (int)mesh->getDimension(), nen = mesh->nodesPerElement(), nv = dim + 1;
        const auto& conn = mesh->connectivity();
        const size_t ne = conn.size() / nen;
        auto mapRep = mesh->getMapRepeated();
        auto mapUni = mesh->getMapUnique();
        nPoints_ = (size_t)mapUni->getGlobalNumElements();
        TEUCHOS_TEST_FOR_EXCEPTION(size > 1 && (GO)nPoints_ <= mapUni->getMaxAllGlobalIndex(), std::logic_error,
                                   "ExporterParaView: node ids are not 0 .. N-1");
        std::vector<char> owned(mapRep->getNodeNumElements(), 0);
        for (int32_t rl : mesh->uniqueLocalOfRepeated()) owned[rl] = 1;
        // connectivity in global ids of the elements this rank exports, vertices only
        std::vector<int32_t> c;
        c.reserve(ne * nv);
        for (size_t e = 0; e < ne; ++e) {
            int jmin = 0;
            for (int j = 1; j < nv; ++j)
                if (mapRep->getGlobalElement(conn[e * nen + j]) < mapRep->getGlobalElement(conn[e * nen + jmin])) jmin = j;
            if (!owned[conn[e * nen + jmin]]) continue;
            for (int j = 0; j < nv; ++j) c.push_back((int32_t)mapRep->getGlobalElement(conn[e * nen + j]));
        }
        std::vector<int64_t> counts = gatherCounts((int64_t)(c.size() / nv));
        int64_t before = 0, total = 0;
        for (int r = 0; r < size; ++r) {
            if (r < rank) before += counts[r];
            total += counts[r];
        }
        nElements_ = (size_t)total;
        createFile(filename_ + ".conn.bin", (size_t)total * nv * sizeof(int32_t));
        writeAt(filename_ + ".conn.bin", (size_t)before * nv * sizeof(int32_t), c.data(), c.size() * sizeof(int32_t));
        // points of the unique nodes, at their global positions
        uniGid_.assign(mapUni->gids().begin(), mapUni->gids().end());
        auto pts = mesh->getPointsUnique();
        std::vector<double> xyz(uniGid_.size() * 3, 0.0);
        for (size_t i = 0; i < uniGid_.size(); ++i)
            for (int d = 0; d < dim; ++d) xyz[i * 3 + d] = (*pts)[i][d];
        createFile(filename_ + ".xyz.bin", nPoints_ * 3 * sizeof(double));
        writeRecords(filename_ + ".xyz.bin", xyz.data(), 3 * sizeof(double));
        comm_->barrier();
        topology_ = dim == 3 ? "Tetrahedron" : "Triangle";
        nv_ = nv;
    }
    void addVariable(MultiVecConstPtr_Type& u, std::string varName, std::string varType, int dofPerNode,
                     MapConstPtr_Type mapUnique = Teuchos::null, MapConstPtr_Type mapUniqueLeading = Teuchos::null) {
        (void)mapUnique; (void)mapUniqueLeading;
        TEUCHOS_TEST_FOR_EXCEPTION(varType != "Scalar" && varType != "Vector", std::logic_error, "Unknown variable type for exporter.");
        TEUCHOS_TEST_FOR_EXCEPTION(u->getLocalLength() != uniGid_.size() * (size_t)dofPerNode, std::logic_error,
                                   "ExporterParaView::addVariable: vector length does not match the mesh");
        vars_.push_back({u, varName, varType, dofPerNode});
    }
    void save(double time) { save(time, 0.); }
    void save(double time, double dt) {
        (void)dt;
        if (timeIndex_ % saveTimestep_ == 0) {
            for (auto& v : vars_) {
                const auto& x = v.u->raw();
                const int comps = v.type == "Vector" ? 3 : 1;
                const size_t nl = uniGid_.size();
                std::vector<double> out(nl * comps, 0.0);
                for (size_t i = 0; i < nl; ++i)
                    for (int d = 0; d < v.dofs && d < comps; ++d) out[i * comps + d] = x[i * v.dofs + d];
                const std::string f = filename_ + "." + v.name + "." + std::to_string(nSaved_) + ".bin";
                createFile(f, nPoints_ * comps * sizeof(double));
                writeRecords(f, out.data(), comps * sizeof(double));
            }
            comm_->barrier();
            times_.push_back(time);
            ++nSaved_;
            if (comm_->getRank() == 0) writeXmf();
        }
        ++timeIndex_;
    }
    void closeExporter() { if (comm_.is_null() || comm_->getRank() == 0) writeXmf(); }
private:
    struct Var { MultiVecConstPtr_Type u; std::string name, type; int dofs; };
    std::vector<int64_t> gatherCounts(int64_t mine) const {
        std::vector<char> all;
        comm_->gatherAll(&mine, sizeof(mine), all);
        std::vector<int64_t> out((size_t)comm_->getSize());
        std::memcpy(out.data(), all.data(), out.size() * sizeof(int64_t));
        return out;
    }
    // rank 0 creates the file at its final size; nobody writes before it exists
    void createFile(const std::string& f, size_t bytes) const {
        if (comm_->getRank() == 0) {
            std::ofstream os(f, std::ios::binary | std::ios::trunc);
            TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: cannot write " << f);
            if (bytes > 0) {
                os.seekp((std::streamoff)bytes - 1);
                os.put('\0');
            }
        }
        comm_->barrier();
    }
    static void writeAt(const std::string& f, size_t offset, const void* p, size_t bytes) {
        if (bytes == 0) return;
        std::fstream os(f, std::ios::binary | std::ios::in | std::ios::out);
        TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: cannot write " << f);
        os.seekp((std::streamoff)offset);
        os.write((const char*)p, (std::streamsize)bytes);
        TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: short write to " << f);
    }
    // record i of `data` (one per unique node) to position gid(i): runs of consecutive global ids go out in one write
    void writeRecords(const std::string& f, const double* data, size_t recBytes) const {
        if (uniGid_.empty()) return;
        std::fstream os(f, std::ios::binary | std::ios::in | std::ios::out);
        TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: cannot write " << f);
        size_t i = 0;
        const size_t n = uniGid_.size();
        while (i < n) {
            size_t j = i + 1;
            while (j < n && uniGid_[j] == uniGid_[j - 1] + 1) ++j;
            os.seekp((std::streamoff)((size_t)uniGid_[i] * recBytes));
            os.write((const char*)data + i * recBytes, (std::streamsize)((j - i) * recBytes));
            i = j;
        }
        TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: short write to " << f);
    }
    static std::string base(const std::string& f) { const size_t p = f.find_last_of('/'); return p == std::string::npos ? f : f.substr(p + 1); }
    void writeXmf() const {
        std::ofstream os(filename_ + ".xmf");
        TEUCHOS_TEST_FOR_EXCEPTION(!os, std::runtime_error, "ExporterParaView: cannot write " << filename_ << ".xmf");
        const std::string b = base(filename_);
        os << "<?xml version=\"1.0\" ?>\n<Xdmf Version=\"2.0\">\n<Domain>\n<Grid Name=\"" << b
           << "\" GridType=\"Collection\" CollectionType=\"Temporal\">\n";
        for (size_t k = 0; k < times_.size(); ++k) {
            os << " <Grid Name=\"step" << k << "\" GridType=\"Uniform\">\n  <Time Value=\"" << times_[k] << "\"/>\n"
               << "  <Topology TopologyType=\"" << topology_ << "\" NumberOfElements=\"" << nElements_ << "\">\n"
               << "   <DataItem Format=\"Binary\" DataType=\"Int\" Precision=\"4\" Endian=\"Little\" Dimensions=\"" << nElements_ << " " << nv_
               << "\">" << b << ".conn.bin</DataItem>\n  </Topology>\n"
               << "  <Geometry GeometryType=\"XYZ\">\n   <DataItem Format=\"Binary\" DataType=\"Float\" Precision=\"8\" Endian=\"Little\" Dimensions=\""
               << nPoints_ << " 3\">" << b << ".xyz.bin</DataItem>\n  </Geometry>\n";
            for (auto& v : vars_) {
                const bool vec = v.type == "Vector";
                os << "  <Attribute Name=\"" << v.name << "\" AttributeType=\"" << (vec ? "Vector" : "Scalar") << "\" Center=\"Node\">\n"
                   << "   <DataItem Format=\"Binary\" DataType=\"Float\" Precision=\"8\" Endian=\"Little\" Dimensions=\"" << nPoints_
                   << (vec ? " 3" : "") << "\">" << b << "." << v.name << "." << k << ".bin</DataItem>\n  </Attribute>\n";
            }
            os << " </Grid>\n";
        }
        os << "</Grid>\n</Domain>\n</Xdmf>\n";
    }
    std::string filename_, FEType_, topology_;
    MeshPtr_Type mesh_;
    Teuchos::RCP<const Teuchos::Comm<int> > comm_;
    std::vector<int64_t> uniGid_;
    std::vector<Var> vars_;
    std::vector<double> times_;
    size_t nPoints_ = 0, nElements_ = 0;
    int nv_ = 0, saveTimestep_ = 1, timeIndex_ = 0, nSaved_ = 0;
};

// device time of the kernel classes of the hot path (HIP events on the library's stream, fedd_timing_*) as children of
// the running stacked timer: the StackedTimer report of the drivers' tails then shows where the GPU time went
inline void addDeviceTimers(const DeviceContextPtr& dev, Teuchos::StackedTimer& st) {
    static const char* names[FEDD_T_COUNT] = {"symbolic", "assemble", "rhs", "dirichlet", "spmv", "schwarz setup", "schwarz apply",
                                             "orthogonalisation", "coarse setup", "coarse apply", "halo", "all-reduce", "spmv setup",
                                             "orthogonalisation: dot sweep", "orthogonalisation: update sweep", "orthogonalisation: fused sweep",
                                             "full park (matrix cores)", "full park", "full gather", "cg pq", "cg xr", "cg rz", "cg p",
                                             "newmark state", "block apply", "multistep state", "block preconditioner B^T",
                                             "newton residual", "newton update", "mesh move", "mesh move check"};
    for (int t = 0; t < FEDD_T_COUNT; ++t) {
        double ms = 0.;
        int64_t n = 0;
        if (fedd_timing_get(dev->ctx, t, &ms, &n) == 0 && n > 0) st.addExternal(std::string("FEDD - device - ") + names[t], 1e-3 * ms, (long)n);
    }
}

}  // namespace FEDD
